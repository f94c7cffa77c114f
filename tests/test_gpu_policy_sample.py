"""The stochastic (tanh-Gaussian) policy head on the device: pp3_policy_sample (csrc/pp3_policy.hip
mlp_sample_kernel) and the fused sampled rollout pp3_rollout_policy_sample (csrc/pp3_env.hip
env_step_kernel<8, true, 8, CULL, true>), both running csrc/pp3_mlp.h sample_head.

Tolerances.  Logits: the project's MLP bound |d| <= 2e-5 (1 + |y|) against export.policy_forward.
Head (raw, action, log_prob): against a float64 recomputation from the device's own f32 logits and
the host's threefry bits, so only the head's f32 arithmetic is measured; normalised error
|d| / (1 + |x|).  Ceilings above which a difference is a bug, not rounding: 1e-5 (raw, action),
1e-4 (log_prob) -- f32 eps 6e-8, the head about ten operations deep, zr divides by a scale >=
min_std.  The asserted bounds are 4 x the largest error measured on an MI355X on these inputs,
rounded up to one digit: see HEAD_BOUND below.
"""
import ctypes as C

import numpy as np
import pytest

import common
from pupperv3_mjx import _abi, _lib, export, rng
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_export import _brax_like_params

pytestmark = pytest.mark.gpu

LO = np.nextafter(np.float32(-1.0), np.float32(0.0))
# measured on an MI355X over the four cases of test_head_matches_numpy and the partitionable = 0
# case (largest normalised error): raw 2.2e-7, action 1.5e-7, log_prob 1.2e-6
HEAD_BOUND = {"raw": 9e-7, "action": 6e-7, "log_prob": 5e-6}


def _training(sizes, act="elu", seed=0, **kw):
    rs = np.random.RandomState(seed)
    return export.convert_training_params(_brax_like_params(rs, sizes), act, 0.75, 5.0, 0.25, np.zeros(12), np.ones(12),
                                          -np.ones(12), True, (sizes[0] // 36), 30.0, 30.0, **kw)


def _download(buf, shape):
    a = np.zeros(shape, dtype=np.float32)
    _lib.check(_lib.load().pp3_memcpy_d2h(a.ctypes.data_as(C.c_void_p), buf.ptr, a.nbytes))
    return a


def _sample(pol, x, key, part=True):
    """One pp3_policy_sample call on rows x: {"action", "raw", "log_prob", "logits"} (float32)."""
    n = x.shape[0]
    dp = export.DevicePolicy(pol)
    bufs = [_lib.DeviceBuffer(x.nbytes)] + [_lib.DeviceBuffer(4 * n * w) for w in (12, 12, 1, 24)]
    try:
        bufs[0].upload(x)
        dp.sample(bufs[0].ptr.value, x.shape[1], n, key, bufs[1].ptr.value, 12, bufs[2].ptr.value, bufs[3].ptr.value,
                  bufs[4].ptr.value, partitionable=part)
        return {"action": _download(bufs[1], (n, 12)), "raw": _download(bufs[2], (n, 12)),
                "log_prob": _download(bufs[3], (n,)), "logits": _download(bufs[4], (n, 24))}
    finally:
        for b in bufs:
            b.free()
        dp.close()


def _recompute(pol, got, key, part):
    """float64 head from the device's f32 logits and the host's bits."""
    from scipy.special import erfinv
    n = got["logits"].shape[0]
    d = pol["distribution"]
    loc, scale = export.normal_tanh_scale(got["logits"], d["min_std"], d["var_scale"])
    u = rng.uniform(key, (n, 12), LO, 1.0, part)
    raw = loc + scale * (np.sqrt(2.0) * erfinv(u.astype(np.float64)))
    return {"raw": raw, "action": np.tanh(raw),
            "log_prob": export.normal_tanh_log_prob(got["logits"], raw, d["min_std"], d["var_scale"])}


def _check_head(pol, x, got, key, part):
    want_logits = export.policy_forward(pol, x.astype(np.float64))
    assert np.all(np.abs(got["logits"] - want_logits) <= 2e-5 * (1 + np.abs(want_logits))), \
        np.abs(got["logits"] - want_logits).max()
    want = _recompute(pol, got, key, part)
    errs = {k: float((np.abs(got[k] - want[k]) / (1 + np.abs(want[k]))).max()) for k in HEAD_BOUND}
    print("head normalised errors", x.shape, "part" if part else "nopart", errs)
    for k, bound in HEAD_BOUND.items():
        assert errs[k] <= bound, (k, errs[k])
    assert np.all(np.abs(got["action"]) <= 1.0)


@pytest.mark.parametrize("sizes,act,n", [([72, 128, 128, 24], "elu", 37), ([72, 64, 24], "sigmoid", 16),
                                         ([72, 128, 128, 24], "tanh", 1), ([540, 256, 24], "relu", 20)])
def test_head_matches_numpy(require_gpu, sizes, act, n):
    """(a) logits against policy_forward; raw / action / log_prob against the float64 head.  Measured
    largest normalised errors (MI355X, these four cases and the partitionable = 0 one): raw 2.2e-7,
    action 1.5e-7, log_prob 1.2e-6; bounds HEAD_BOUND = 4 x those, rounded up to one digit: 9e-7,
    6e-7, 5e-6 (the ceilings for rounding are 1e-5, 1e-5, 1e-4)."""
    pol = _training(sizes, act)
    x = np.random.RandomState(1).normal(size=(n, sizes[0])).astype(np.float32)
    key = rng.PRNGKey(3)
    _check_head(pol, x, _sample(pol, x, key), key, True)


def test_head_extremes_stay_finite(require_gpu):
    """+-20 on the bias of a few scale columns (scale ~ 20 and scale ~ min_std), +-15 on a few loc
    columns (saturated tanh): everything finite, |action| <= 1."""
    pol = _training([72, 128, 128, 24])
    b = pol["layers"][-1]["weights"][1]
    for col, add in ((12, 20.0), (13, 20.0), (14, -20.0), (15, -20.0), (0, 15.0), (1, -15.0), (2, 15.0)):
        b[col] += add
    n = 37
    x = np.random.RandomState(1).normal(size=(n, 72)).astype(np.float32)
    got = _sample(pol, x, rng.PRNGKey(4))
    for k, v in got.items():
        assert np.all(np.isfinite(v)), k
    assert np.all(np.abs(got["action"]) <= 1.0)
    _, scale = export.normal_tanh_scale(got["logits"])
    assert scale[:, 0].min() > 10 and scale[:, 2].max() < 0.002  # the cases are what they claim to be
    assert np.abs(got["action"][:, 2]).min() > 0.999  # loc +15 with scale ~ min_std: saturated


def test_sampling_is_a_function_of_the_key_and_the_row(require_gpu):
    """(b) the same key twice: the same bits; another key: another raw; the word of (env, j) is
    element env * 12 + j whatever n is (partitionable): rows 0..15 of an n = 37 call equal an
    n = 16 call on the same rows bit for bit."""
    pol = _training([72, 128, 128, 24])
    x = np.random.RandomState(1).normal(size=(37, 72)).astype(np.float32)
    a, b = _sample(pol, x, rng.PRNGKey(3)), _sample(pol, x, rng.PRNGKey(3))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    c = _sample(pol, x, rng.PRNGKey(4))
    np.testing.assert_array_equal(a["logits"], c["logits"])
    assert np.all(a["raw"] != c["raw"])
    d = _sample(pol, x[:16], rng.PRNGKey(3))
    for k in a:
        np.testing.assert_array_equal(a[k][:16], d[k])


def test_head_non_partitionable_stream(require_gpu):
    """(b) rng_partitionable = 0 (the pre-0.5 counter layout, whose words depend on n): the
    tolerance check of (a) at n = 37."""
    pol = _training([72, 128, 128, 24])
    x = np.random.RandomState(1).normal(size=(37, 72)).astype(np.float32)
    key = rng.PRNGKey(3)
    got = _sample(pol, x, key, part=False)
    _check_head(pol, x, got, key, False)
    assert np.all(got["raw"] != _sample(pol, x, key, part=True)["raw"])


def _loop_reference(w, env, st, dp, K, key, part=True):
    """The per-step Python loop: DevicePolicy.sample_env (the stand-alone kernel) with the host's
    split chain, then step.  Returns (state, traj, K_nsteps)."""
    n = env.num_envs
    bufs = [_lib.DeviceBuffer(4 * n * w_) for w_ in (12, 12, 1)]
    out = {k: [] for k in ("action", "raw_action", "log_prob", "obs", "reward", "done")}
    try:
        for _ in range(K):
            cur, key = rng.split(key, 2, part)
            dp.sample_env(env, cur, bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value)
            env.synchronize()
            a = _download(bufs[0], (n, 12))
            out["action"].append(a)
            out["raw_action"].append(_download(bufs[1], (n, 12)))
            out["log_prob"].append(_download(bufs[2], (n,)))
            st = w.step(st, a)
            out["obs"].append(np.array(st.obs)); out["reward"].append(np.array(st.reward)); out["done"].append(np.array(st.done))
    finally:
        for b in bufs:
            b.free()
    return st, {k: np.stack(v) for k, v in out.items()}, key


def _assert_same(tr, ref):
    for k in ("action", "raw_action", "log_prob", "obs", "reward", "done"):
        np.testing.assert_array_equal(tr[k], ref[k], err_msg=k)


@pytest.mark.parametrize("n,sizes,H,K", [(48, [72, 128, 128, 24], 2, 12), (37, [72, 256, 128, 128, 24], 2, 12),
                                         (1, [72, 128, 128, 24], 2, 12), (20, [540, 256, 128, 24], 15, 6)])
def test_rollout_policy_sample_equals_sample_then_step(require_gpu, tmp_path, n, sizes, H, K):
    """(c) pp3_rollout_policy_sample (ONE fused launch, the head inside the workgroup's MLP, the key
    chain advanced on the device) equals the per-step loop bit for bit, auto-reset inside the
    window; ragged workgroups (37, 1 envs) and observation_history 15 (obs from global memory)."""
    from pupperv3_mjx import wrappers
    path = common.write_model(tmp_path, 0)
    envs = [PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.25, observation_history=H), num_envs=n)
            for _ in range(2)]
    dp = export.DevicePolicy(_training(sizes))
    try:
        assert envs[0]._L.pp3_rollout_policy_fused(envs[0]._h) == 1
        ws = [wrappers.wrap(e, episode_length=5) for e in envs]
        s1, s2 = ws[0].reset(make_keys(2, n)), ws[1].reset(make_keys(2, n))
        key = rng.PRNGKey(9)
        s1, tr, k1 = ws[0].rollout_policy_sample(s1, dp, K, key)
        s2, ref, k2 = _loop_reference(ws[1], envs[1], s2, dp, K, key)
        assert tr["raw_action"].shape == (K, n, 12) and tr["log_prob"].shape == (K, n)
        _assert_same(tr, ref)
        assert tr["done"].sum() > 0 or n == 1
        np.testing.assert_array_equal(s1._record, s2._record)
        np.testing.assert_array_equal(k1, k2)
        assert np.all(np.isfinite(tr["log_prob"])) and np.all(np.abs(tr["action"]) <= 1)
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_chained_unrolls_equal_one(require_gpu, tmp_path):
    """(c) two unrolls of 6, the second from the first's returned key, equal one of 12."""
    from pupperv3_mjx import wrappers
    path = common.write_model(tmp_path, 0)
    n = 20
    envs = [PupperV3Env(**common.fixture_kwargs(path, terminal_body_z=0.25), num_envs=n) for _ in range(2)]
    dp = export.DevicePolicy(_training([72, 64, 24]))
    try:
        ws = [wrappers.wrap(e, episode_length=5) for e in envs]
        s1, s2 = ws[0].reset(make_keys(2, n)), ws[1].reset(make_keys(2, n))
        key = rng.PRNGKey(10)
        s1, tr, k1 = ws[0].rollout_policy_sample(s1, dp, 12, key)
        s2, ta, ka = ws[1].rollout_policy_sample(s2, dp, 6, key)
        ta = {k: np.array(v) for k, v in ta.items()}
        s2, tb, kb = ws[1].rollout_policy_sample(s2, dp, 6, ka)
        _assert_same(tr, {k: np.concatenate([ta[k], tb[k]]) for k in ta})
        np.testing.assert_array_equal(s1._record, s2._record)
        np.testing.assert_array_equal(k1, kb)
        assert not np.array_equal(ka, kb)
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_non_partitionable_env_chain(require_gpu, tmp_path):
    """(c) rng_partitionable = False: the key chain's split and the head's words take the pre-0.5
    layout in the fused kernel, in the stand-alone one and on the host alike."""
    path = common.write_model(tmp_path, 0)
    n, K = 20, 4
    envs = [PupperV3Env(**common.fixture_kwargs(path), num_envs=n, rng_partitionable=False) for _ in range(2)]
    dp = export.DevicePolicy(_training([72, 64, 24]))
    try:
        assert envs[0]._L.pp3_rollout_policy_fused(envs[0]._h) == 1
        s1, s2 = envs[0].reset(make_keys(2, n, False)), envs[1].reset(make_keys(2, n, False))
        key = rng.PRNGKey(14)
        s1, tr, k1 = envs[0].rollout_policy_sample(s1, dp, K, key)
        s2, ref, k2 = _loop_reference(envs[1], envs[1], s2, dp, K, key, part=False)
        _assert_same(tr, ref)
        np.testing.assert_array_equal(s1._record, s2._record)
        np.testing.assert_array_equal(k1, k2)
        k = key
        for _ in range(K):
            k = rng.split(k, 2, False)[1]
        np.testing.assert_array_equal(k1, k)
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_unfused_fallback_equals_loop(require_gpu, tmp_path):
    """(c) max_contacts = 16: per step a sample launch with that step's key, then a step launch."""
    path = common.write_model(tmp_path, 0)
    n, K = 20, 4
    envs = [PupperV3Env(**common.fixture_kwargs(path), num_envs=n, max_contacts=16) for _ in range(2)]
    dp = export.DevicePolicy(_training([72, 64, 24]))
    try:
        assert envs[0]._L.pp3_rollout_policy_fused(envs[0]._h) == 0
        s1, s2 = envs[0].reset(make_keys(2, n)), envs[1].reset(make_keys(2, n))
        key = rng.PRNGKey(12)
        s1, tr, k1 = envs[0].rollout_policy_sample(s1, dp, K, key)
        s2, ref, k2 = _loop_reference(envs[1], envs[1], s2, dp, K, key)
        _assert_same(tr, ref)
        np.testing.assert_array_equal(s1._record, s2._record)
        np.testing.assert_array_equal(k1, k2)
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_rollout_policy_sample_with_dr_and_terrain(require_gpu, tmp_path):
    """(c) domain-randomised envs on per-env terrain (the CULL instantiation, 16 envs per workgroup
    and a tail workgroup at n = 40): bit-equal to the per-step loop."""
    from pupperv3_mjx import domain_randomization
    path = common.write_model(tmp_path, 10)
    n, K = 40, 6
    envs = [PupperV3Env(**common.fixture_kwargs(path), num_envs=n) for _ in range(2)]
    dp = export.DevicePolicy(_training([72, 256, 128, 128, 24]))
    try:
        sysb, _ = domain_randomization.domain_randomize(envs[0].sys, rng.split(rng.PRNGKey(3), n))
        states = []
        for e in envs:
            e.set_domain_randomization(sysb)
            st = e.reset(make_keys(4, n))
            xy = st._record[:, _abi.S_QPOS:_abi.S_QPOS + 2].astype(np.float64)
            e.set_terrain(common.terrain_under(xy, 10, seed=5))
            states.append(st)
        key = rng.PRNGKey(13)
        s1, tr, k1 = envs[0].rollout_policy_sample(states[0], dp, K, key)
        s2, ref, k2 = _loop_reference(envs[1], envs[1], states[1], dp, K, key)
        _assert_same(tr, ref)
        np.testing.assert_array_equal(s1._record, s2._record)
        np.testing.assert_array_equal(k1, k2)
        assert s1.pipeline_state.contact.ncon.sum() > 0
    finally:
        dp.close()
        for e in envs:
            e.close()


def test_device_noise_moments(require_gpu):
    """(d) n = 512 from PRNGKey(11), one call: (raw - loc) / scale recovered from the returned
    logits has mean and variance within four standard errors (+ 1e-3 for the f32 round trip), and
    adjacent action columns are uncorrelated (|r| < 4 / sqrt(512))."""
    pol = _training([72, 64, 24])
    n = 512
    x = np.random.RandomState(1).normal(size=(n, 72)).astype(np.float32)
    got = _sample(pol, x, rng.PRNGKey(11))
    loc, scale = export.normal_tanh_scale(got["logits"])
    z = (got["raw"].astype(np.float64) - loc) / scale
    assert abs(z.mean()) <= 4 / np.sqrt(n * 12) + 1e-3, z.mean()
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / (n * 12)) + 1e-3, z.var()
    for j in range(11):
        r = np.corrcoef(z[:, j], z[:, j + 1])[0, 1]
        assert abs(r) < 4 / np.sqrt(n), (j, r)
