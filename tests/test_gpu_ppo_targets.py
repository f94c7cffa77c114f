"""On-device PPO collection: per-step truncation rows (pp3_set_truncation_trajectory, csrc/pp3_env.hip
env_step_kernel), the critic through pp3_policy_act, GAE value targets (pp3_gae, csrc/pp3_ppo.hip)
and PupperV3Env.collect_ppo.

Everything but the critic's values is compared bit for bit: pp3_gae against the f32 restatement of
its recurrence (tests/ppo_ref.py), truncation rows against the single-step record.  The critic uses
the project's MLP bound |d| <= 2e-5 (1 + |y|) against export.policy_forward in float64."""
import ctypes as C

import numpy as np
import pytest

import common
import ppo_ref
from pupperv3_mjx import _abi, _lib, export, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys
from test_export import _brax_like_params

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
TINY = np.finfo(np.float32).tiny


def _download(ptr, shape):
    a = np.zeros(shape, dtype=np.float32)
    _lib.check(_lib.load().pp3_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes))
    return a


def _training(sizes, seed=0):
    rs = np.random.RandomState(seed)
    return export.convert_training_params(_brax_like_params(rs, sizes), "elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12),
                                          -np.ones(12), True, sizes[0] // 36, 30.0, 30.0)


def _value(sizes, act="elu", seed=5):
    return export.convert_value_params(_brax_like_params(np.random.RandomState(seed), sizes), act, sizes[0] // 36)


# ------------------------------------------------------------------------------ pp3_gae
GAE_SHAPES = [(1, 1, 1), (2, 63, 63), (7, 64, 64), (7, 65, 80), (5, 257, 257)]


def _gae_inputs(K, N, seed):
    """rewards U(0, 0.05), values / bootstrap N(0, 3), done p = 0.3 (1 in column 0 at t = 0 and
    t = K - 1), truncation = done & Bernoulli(0.5); column 1 all done, column 2 all truncated."""
    rs = np.random.RandomState(seed)
    reward = rs.uniform(0, 0.05, size=(K, N)).astype(np.float32)
    values = rs.normal(scale=3.0, size=(K, N)).astype(np.float32)
    bootstrap = rs.normal(scale=3.0, size=N).astype(np.float32)
    done = (rs.uniform(size=(K, N)) < 0.3).astype(np.float32)
    done[0, 0] = done[K - 1, 0] = 1
    coin = (rs.uniform(size=(K, N)) < 0.5).astype(np.float32)
    if N > 1:
        done[:, 1] = 1
    if N > 2:
        done[:, 2] = 1
        coin[:, 2] = 1
    return reward, done, done * coin, values, bootstrap


@pytest.mark.parametrize("discount,lam,scaling", [(0.97, 0.95, 1.0), (0.5, 0.0, 2.0), (1.0, 1.0, 0.1)])
def test_gae_equals_the_f32_restatement_bit_for_bit(require_gpu, discount, lam, scaling):
    L = require_gpu
    kinds = np.zeros(2, dtype=int)  # (done = 1, trunc = 0) and (done = 1, trunc = 1) steps over the shapes
    for si, (K, N, stride) in enumerate(GAE_SHAPES):
        ins = _gae_inputs(K, N, seed=10 + si)
        reward, done, trunc, values, bootstrap = ins
        kinds += [int(((done == 1) & (trunc == 0)).sum()), int(((done == 1) & (trunc == 1)).sum())]
        inter = []
        want_vs, want_adv = ppo_ref.gae(*ins, discount, lam, scaling, intermediates=inter)
        for a in inter:  # the device flushes subnormals, numpy does not: the inputs must keep clear of them
            assert not np.any((a != 0) & (np.abs(a) < TINY))
        bufs = []
        try:
            for a in (reward, done, trunc, values):  # pad columns beyond N hold the sentinel
                padded = np.full((K, stride), SENTINEL, np.float32)
                padded[:, :N] = a
                bufs.append(_lib.DeviceBuffer(padded.nbytes))
                bufs[-1].upload(padded)
            bufs.append(_lib.DeviceBuffer(bootstrap.nbytes))
            bufs[-1].upload(bootstrap)
            for _ in range(2):  # vs, adv
                bufs.append(_lib.DeviceBuffer(4 * K * stride))
                bufs[-1].upload(np.full((K, stride), SENTINEL, np.float32))
            p = [b.ptr for b in bufs]
            rc = L.pp3_gae(0, K, N, stride, p[0], p[1], p[2], p[3], p[4], discount, lam, scaling, p[5], p[6], None)
            assert rc == 0, L.pp3_ppo_last_error()
            vs, adv = _download(p[5].value, (K, stride)), _download(p[6].value, (K, stride))
        finally:
            for b in bufs:
                b.free()
        for got, want, name in ((vs, want_vs, "vs"), (adv, want_adv, "adv")):
            np.testing.assert_array_equal(got[:, :N], want, err_msg=f"{name} {(K, N, stride)}")
            assert np.all(got[:, N:] == SENTINEL), (name, K, N, stride)
            assert np.all(got[:, :N] != SENTINEL), (name, K, N, stride)
    assert kinds[0] >= 1 and kinds[1] >= 1, kinds


def test_gae_refuses_aliased_outputs_on_the_device(require_gpu):
    L = require_gpu
    b = [_lib.DeviceBuffer(4 * 8) for _ in range(6)]
    try:
        p = [x.ptr for x in b]
        assert L.pp3_gae(0, 2, 4, 4, p[0], p[1], p[2], p[3], p[4], 0.9, 0.9, 1.0, p[3], p[5], None) == 1
        assert b"in-place" in L.pp3_ppo_last_error()
    finally:
        for x in b:
            x.free()


# ------------------------------------------------------------------------------ truncation rows
def _twins(tmp_path, n, count=2, **over):
    path = common.write_model(tmp_path, 0)
    over.setdefault("terminal_body_z", 0.21)  # start heights are 0.18 .. 0.24: some envs end at once, others live
    return [PupperV3Env(**common.fixture_kwargs(path, **over), num_envs=n) for _ in range(count)]


def _step_record(w, st, actions):
    """K wrapper steps one by one: (state, truncation [K, N], done [K, N]) read after each step."""
    tr, dn = [], []
    for a in actions:
        st = w.step(st, a)
        tr.append(np.array(st.info["truncation"], dtype=np.float32))
        dn.append(np.array(st.done, dtype=np.float32))
    return st, np.stack(tr), np.stack(dn)


def _compare_truncation(tmp_path, n, K, flavour="actions", episode_length=3, action_repeat=1, **over):
    envs = _twins(tmp_path, n, **over)
    dp = export.DevicePolicy(_training([72, 64, 24])) if flavour == "sample" else \
        export.DevicePolicy(export.convert_params(_brax_like_params(np.random.RandomState(0), [72, 64, 24]), "elu", 0.75,
                                                  5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12), True, 2, 30.0,
                                                  30.0)) if flavour == "policy" else None
    try:
        ws = [wrappers.wrap(e, episode_length=episode_length, action_repeat=action_repeat) for e in envs]
        s1, s2 = ws[0].reset(make_keys(2, n)), ws[1].reset(make_keys(2, n))
        if flavour == "actions":
            acts = np.random.RandomState(7).uniform(-1, 1, size=(K, n, 12)).astype(np.float32)
            s1, traj = ws[0].rollout(s1, acts, truncation=True)
        elif flavour == "policy":
            s1, traj = ws[0].rollout_policy(s1, dp, K, truncation=True)
            acts = np.array(traj["action"])
        else:
            s1, traj, _ = ws[0].rollout_policy_sample(s1, dp, K, rng.PRNGKey(9), truncation=True)
            acts = np.array(traj["action"])
        assert traj["truncation"].shape == (K, n)
        s2, want_tr, want_done = _step_record(ws[1], s2, acts)
        np.testing.assert_array_equal(traj["truncation"], want_tr)
        np.testing.assert_array_equal(traj["done"], want_done)
        np.testing.assert_array_equal(s1._record, s2._record)
        assert envs[0]._L.pp3_rollout_policy_fused(envs[0]._h) == (0 if "max_contacts" in over or action_repeat > 1 else 1)
        return np.array(traj["truncation"]), np.array(traj["done"])
    finally:
        if dp is not None:
            dp.close()
        for e in envs:
            e.close()


def test_truncation_rows_equal_the_single_step_record(require_gpu, tmp_path):
    """N = 6, K = 8, episode_length 3: both kinds of episode end are in the window, and `done`
    alone does not tell them apart."""
    tr, done = _compare_truncation(tmp_path, 6, 8)
    assert np.all(done[tr == 1] == 1)
    assert (tr == 1).sum() >= 1
    assert ((done == 1) & (tr == 0)).sum() >= 1


@pytest.mark.parametrize("n,K,flavour,kw", [
    (6, 1, "actions", {}),                      # the single-step kernel
    (5, 8, "actions", {}),                      # an odd batch: the last half-wave stores nothing
    (17, 8, "policy", {}),                      # a tail workgroup of the 16-env policy launch
    (17, 8, "sample", {}),
    (6, 8, "actions", {"max_contacts": 16}),    # per-step launches
    (6, 8, "policy", {"max_contacts": 16}),
    (6, 8, "sample", {"max_contacts": 16}),
    (6, 4, "actions", {"episode_length": 8, "action_repeat": 3}),  # truncation at wrapper step 3
    (6, 4, "sample", {"episode_length": 8, "action_repeat": 3}),
], ids=["k1", "odd_n", "policy_tail", "sample_tail", "nc16", "nc16_policy", "nc16_sample", "repeat3", "repeat3_sample"])
def test_truncation_rows_on_every_launch_path(require_gpu, tmp_path, n, K, flavour, kw):
    tr, done = _compare_truncation(tmp_path, n, K, flavour, **kw)
    assert np.all(done[tr == 1] == 1)
    if kw.get("action_repeat") == 3:  # 3, 6, 9 >= 8 env steps: no truncation before wrapper step 3
        assert not tr[:2].any()


def test_truncation_rows_are_zero_without_auto_reset(require_gpu, tmp_path):
    n, K = 6, 3
    env = _twins(tmp_path, n, count=1)[0]
    buf = _lib.DeviceBuffer(4 * K * n)
    try:
        st = env.reset(make_keys(2, n))
        buf.upload(np.full((K, n), SENTINEL, np.float32))
        _lib.check(env._L.pp3_set_truncation_trajectory(env._h, buf.ptr, K))
        acts = np.random.RandomState(7).uniform(-1, 1, size=(K, n, 12)).astype(np.float32)
        st, traj = env.rollout(st, acts)
        assert "truncation" not in traj
        np.testing.assert_array_equal(_download(buf.ptr.value, (K, n)), np.zeros((K, n), np.float32))
        _lib.check(env._L.pp3_set_truncation_trajectory(env._h, None, 0))
        st, traj = env.rollout(st, acts, truncation=True)
        np.testing.assert_array_equal(traj["truncation"], np.zeros((K, n), np.float32))
    finally:
        env.close()
        buf.free()


def test_truncation_capacity_is_checked_before_any_launch(require_gpu, tmp_path):
    n = 6
    env = _twins(tmp_path, n, count=1)[0]
    buf, act = _lib.DeviceBuffer(4 * 2 * n), _lib.DeviceBuffer(4 * 3 * n * 12)
    dp = export.DevicePolicy(_training([72, 64, 24]))
    try:
        w = wrappers.wrap(env, episode_length=3)
        w.reset(make_keys(2, n))
        act.upload(np.random.RandomState(7).uniform(-1, 1, size=(3, n, 12)).astype(np.float32))
        fields = (_abi.F_STATE, _abi.F_OBS, _abi.F_REWARD, _abi.F_DONE, _abi.F_EPISODE)
        before = [env._get(f).view(np.uint32) for f in fields]
        _lib.check(env._L.pp3_set_truncation_trajectory(env._h, buf.ptr, 2))
        assert env._L.pp3_rollout(env._h, act.ptr, n * 12, 3, None, None, None, None) == 1
        assert b"max_steps" in env._L.pp3_last_error()
        assert env._L.pp3_rollout_policy(env._h, dp._h, 3, act.ptr, None, None, None, None) == 1
        k = np.array([1, 2], np.uint32)
        ko = np.zeros(2, np.uint32)
        assert env._L.pp3_rollout_policy_sample(env._h, dp._h, 3, k.ctypes.data_as(C.c_void_p), ko.ctypes.data_as(C.c_void_p),
                                                act.ptr, None, None, None, None, None, None) == 1
        env.synchronize()
        for f, b in zip(fields, before):
            np.testing.assert_array_equal(env._get(f).view(np.uint32), b)
        _lib.check(env._L.pp3_set_truncation_trajectory(env._h, None, 0))
    finally:
        dp.close()
        env.close()
        buf.free()
        act.free()


def test_unregistered_rollout_is_unchanged(require_gpu, tmp_path):
    """6 envs x 4 steps of rollout_policy_sample with and without the truncation row: every other
    output and the final state record are bit-equal."""
    n, K = 6, 4
    envs = _twins(tmp_path, n)
    dp = export.DevicePolicy(_training([72, 64, 24]))
    try:
        ws = [wrappers.wrap(e, episode_length=3) for e in envs]
        s1, s2 = ws[0].reset(make_keys(2, n)), ws[1].reset(make_keys(2, n))
        s1, a, k1 = ws[0].rollout_policy_sample(s1, dp, K, rng.PRNGKey(9))
        s2, b, k2 = ws[1].rollout_policy_sample(s2, dp, K, rng.PRNGKey(9), truncation=True)
        assert set(b) == set(a) | {"truncation"}
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(s1._record.view(np.uint32), s2._record.view(np.uint32))
        np.testing.assert_array_equal(k1, k2)
        for f in (_abi.F_STATE, _abi.F_EPISODE, _abi.F_METRICS):
            np.testing.assert_array_equal(envs[0]._get(f).view(np.uint32), envs[1]._get(f).view(np.uint32))
    finally:
        dp.close()
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------ the critic
def _act_rows(dp, x):
    """pp3_policy_act with action_stride 1 on rows x: values [n]; the floats behind them keep a sentinel."""
    n = x.shape[0]
    xin, out = _lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(4 * (n + 16))
    try:
        xin.upload(x)
        out.upload(np.full(n + 16, SENTINEL, np.float32))
        dp.act(xin.ptr.value, x.shape[1], n, out.ptr.value, 1)
        got = _download(out.ptr.value, (n + 16,))
        assert np.all(got[n:] == SENTINEL)
        return got[:n]
    finally:
        xin.free()
        out.free()


@pytest.mark.parametrize("sizes,act", [([72, 64, 64, 1], "elu"), ([540, 256, 1], "relu")])
def test_critic_values_match_policy_forward(require_gpu, sizes, act):
    v = _value(sizes, act)
    dp = export.DevicePolicy(v)
    try:
        x = np.random.RandomState(1).normal(size=(37, sizes[0])).astype(np.float32)
        got = _act_rows(dp, x)
        want = export.policy_forward(v, x.astype(np.float64))[:, 0]
        err = np.abs(got - want)
        print("critic max |d| / (1 + |y|)", sizes, float((err / (1 + np.abs(want))).max()))
        assert np.all(err <= 2e-5 * (1 + np.abs(want))), err.max()
    finally:
        dp.close()


# ------------------------------------------------------------------------------ collect_ppo
PER_STEP = ("observation", "obs", "action", "raw_action", "log_prob", "reward", "done", "truncation", "value")


def test_collect_ppo_end_to_end(require_gpu, tmp_path):
    n, K = 6, 5
    disc, lam, scale = 0.97, 0.95, 0.5
    envs = _twins(tmp_path, n, count=3)
    dp, vp = export.DevicePolicy(_training([72, 64, 24])), export.DevicePolicy(_value([72, 64, 64, 1]))
    try:
        ws = [wrappers.wrap(e, episode_length=3) for e in envs]
        s = [w.reset(make_keys(2, n)) for w in ws]
        start_obs = np.array(s[0].obs)
        key = rng.PRNGKey(9)
        s0, batch, k0 = ws[0].collect_ppo(s[0], dp, vp, K, key, disc, lam, scale)
        s1, ref, k1 = ws[1].rollout_policy_sample(s[1], dp, K, key, truncation=True)
        # the unroll is rollout_policy_sample's
        for k in ref:
            np.testing.assert_array_equal(batch[k], ref[k], err_msg=k)
        np.testing.assert_array_equal(s0._record.view(np.uint32), s1._record.view(np.uint32))
        np.testing.assert_array_equal(np.array(s0.obs), np.array(s1.obs))
        np.testing.assert_array_equal(k0, k1)
        assert (batch["truncation"] == 1).sum() >= 1 and ((batch["done"] == 1) & (batch["truncation"] == 0)).sum() >= 1
        # the observation rows
        assert batch["observation"].shape == (K, n, 72) and batch["value"].shape == (K, n)
        assert batch["bootstrap_value"].shape == (n,) and batch["value_target"].shape == (K, n)
        np.testing.assert_array_equal(batch["observation"][0], start_obs)
        np.testing.assert_array_equal(batch["observation"][1:], batch["obs"][:-1])
        # the critic on the returned observations
        rows = np.concatenate([batch["observation"], batch["obs"][-1:]]).reshape((K + 1) * n, 72)
        vals = _act_rows(vp, np.ascontiguousarray(rows)).reshape(K + 1, n)
        np.testing.assert_array_equal(batch["value"], vals[:K])
        np.testing.assert_array_equal(batch["bootstrap_value"], vals[K])
        # the targets from the returned rows
        vs, adv = ppo_ref.gae(batch["reward"], batch["done"], batch["truncation"], batch["value"],
                              batch["bootstrap_value"], disc, lam, scale)
        np.testing.assert_array_equal(batch["value_target"], vs)
        np.testing.assert_array_equal(batch["advantage"], adv)
        # the device addresses hold the same arrays
        dev = ws[0].ppo_device_batch()
        assert set(dev) == set(batch)
        for k, (ptr, shape) in dev.items():
            np.testing.assert_array_equal(_download(ptr, shape), batch[k], err_msg=k)
        # two chained collections of 2 and 3 steps: the same rows
        s2, ba, ka = ws[2].collect_ppo(s[2], dp, vp, 2, key, disc, lam, scale)
        ba = {k: np.array(v) for k, v in ba.items()}
        s2, bb, kb = ws[2].collect_ppo(s2, dp, vp, 3, ka, disc, lam, scale)
        for k in PER_STEP:
            np.testing.assert_array_equal(np.concatenate([ba[k], bb[k]]), batch[k], err_msg=k)
        np.testing.assert_array_equal(bb["bootstrap_value"], batch["bootstrap_value"])
        np.testing.assert_array_equal(s2._record.view(np.uint32), s0._record.view(np.uint32))
        np.testing.assert_array_equal(kb, k0)
    finally:
        dp.close()
        vp.close()
        for e in envs:
            e.close()
