"""Network initialisation on the device (pp3_learner_init_params, csrc/pp3_learn.hip) against its
numpy restatement ppo.init_params bit for bit, in both jax_threefry_partitionable layouts; its reset of
the gradients, moments, step count and normaliser; its refusals; and ppo.make_learner end to end."""
import ctypes as C

import numpy as np
import pytest

import common
from pupperv3_mjx import _abi, export, ppo, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
D = 72
# (policy hidden, value hidden): 5 x 3 and 7 x 1 kernels have odd element counts (the padded counter
# layout of partitionable = False); 73 * 256 + 257 * 24 = 24856 blob elements are 97 full workgroups
# of 256 threads and a ragged one of 24
NETS = {"odd": ((5, 3), (7,)), "wide": ((256,), (256,))}


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _flat(layers):
    return np.concatenate([a.ravel() for kb in layers for a in kb])


def _want(key, hidden, part):
    k_policy, k_value = rng.split(np.asarray(key, U), 2, part)
    return (_flat(ppo.init_params(k_policy, D, hidden[0], 2 * _abi.NU, part)),
            _flat(ppo.init_params(k_value, D, hidden[1], 1, part)))


def _blobs(learner):
    """{(net, which): bits} of all eight blobs (parameters, gradients, m, v of both nets)"""
    return {(n, w): learner._download(n, w).view(U) for n in (0, 1) for w in range(4)}


def _zero_learner(hidden, **kw):
    pol, val = export.zero_network_dicts(D, hidden[0], hidden[1])
    return ppo.PPOLearner(pol, val, max_rows=64, **kw)


@pytest.mark.parametrize("part", [True, False], ids=["partitionable", "legacy"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_init_params_equals_the_restatement_bitwise(require_gpu, name, part):
    hidden = NETS[name]
    learner = _zero_learner(hidden)
    try:
        key = rng.PRNGKey(41)
        learner.init_params(key, part)
        got = _blobs(learner)
        want = _want(key, hidden, part)
        for net in (0, 1):
            assert got[net, 0].size == want[net].size
            np.testing.assert_array_equal(got[net, 0], _bits(want[net]), err_msg=f"net {net}")
            assert np.count_nonzero(got[net, 0]) > 0.9 * (want[net].size - sum(hidden[net]) - (24, 1)[net])
            for which in (1, 2, 3):
                assert not got[net, which].any()
        # params() cuts the blob into the restatement's layers: kernels in [-s, s), biases zero
        for (k, b) in learner.params()["policy"]:
            s = np.sqrt(F(3.0) * (F(1.0) / F(k.shape[0])))
            assert np.all(k >= -s) and np.all(k < s) and not b.any()
        # another key: other bits; the first key again: the first bits
        learner.init_params(rng.PRNGKey(42), part)
        other = _blobs(learner)
        assert all(np.mean(other[net, 0] != got[net, 0]) > 0.9 for net in (0, 1))
        learner.init_params(key, part)
        again = _blobs(learner)
        assert all(np.array_equal(again[k], got[k]) for k in got)
    finally:
        learner.close()


def test_null_arguments_are_refused_and_touch_nothing(require_gpu):
    L = require_gpu
    learner = _zero_learner(NETS["odd"])
    try:
        learner.init_params(rng.PRNGKey(1))
        before = _blobs(learner)
        key = np.array([3, 4], U)
        assert L.pp3_learner_init_params(learner._h, None, 1, None) == _abi.ERR_ARG
        assert b"pp3_learner_init_params" in L.pp3_learn_last_error()
        assert L.pp3_learner_init_params(None, key.ctypes.data_as(C.c_void_p), 1, None) == _abi.ERR_ARG
        after = _blobs(learner)
        assert all(np.array_equal(after[k], before[k]) for k in before)
    finally:
        learner.close()


def test_make_learner_trains_and_init_params_starts_over(require_gpu, tmp_path):
    """make_learner -> make_policies -> train_iteration at 6 envs, K = 3: finite metrics; the step has
    made the gradients, the moments, t and the normaliser non-trivial, and a second init_params with
    the same key returns all of them to the state make_learner left, bit for bit."""
    n, K = 6, 3
    key = rng.PRNGKey(5)
    meta = dict(action_scale=0.75, kp=5.0, kd=0.25, default_pose=np.zeros(12), joint_upper_limits=np.ones(12),
                joint_lower_limits=-np.ones(12), use_imu=True, observation_history=2, maximum_pitch_command=30.0,
                maximum_roll_command=30.0)
    path = common.write_model(tmp_path, 0)
    env = PupperV3Env(**common.fixture_kwargs(path, observation_history=2), num_envs=n)
    learner = ppo.make_learner(key, D, (16, 8), (12,), max_rows=(K + 1) * n, **meta)
    handles = []
    try:
        assert learner.t == 0 and learner.running_statistics
        fresh = _blobs(learner)
        want = _want(key, ((16, 8), (12,)), True)
        for net in (0, 1):
            np.testing.assert_array_equal(fresh[net, 0], _bits(want[net]))
        ns0 = learner.normalizer_state()
        assert ns0["count"] == 0 and not ns0["mean"].any() and np.all(ns0["std"] == 1) and not ns0["summed_variance"].any()
        actor, critic = learner.make_policies()
        handles += [actor, critic]
        w = wrappers.wrap(env, episode_length=5)
        state = w.reset(make_keys(2, n))
        state, metrics, _ = learner.train_iteration(w, state, rng.PRNGKey(9), actor, critic, K, num_minibatches=2,
                                                    shuffle=True, max_grad_norm=1.0, update_normalizer=True,
                                                    device_rng=True)
        assert set(metrics) == set(ppo.METRICS) and all(np.isfinite(v) for v in metrics.values()), metrics
        used = _blobs(learner)
        for net in (0, 1):
            assert np.any(used[net, 0] != fresh[net, 0])
            assert all(used[net, which].any() for which in (1, 2, 3))
        ns = learner.normalizer_state()
        assert learner.t == 2 and ns["count"] == K * n and ns["mean"].any()
        dp = learner.deterministic_policy()  # the export metadata rides along
        handles.append(dp)
        assert dp.out_dim == _abi.NU
        learner.init_params(key)
        back = _blobs(learner)
        assert all(np.array_equal(back[k], fresh[k]) for k in fresh)
        ns1 = learner.normalizer_state()
        assert learner.t == 0 and ns1["count"] == 0
        for k in ("mean", "std", "summed_variance"):
            np.testing.assert_array_equal(_bits(ns1[k]), _bits(ns0[k]))
        # and the learner trains again from there exactly as it did the first time
        learner.sync(actor, critic)
        state = w.reset(make_keys(2, n))
        learner.train_iteration(w, state, rng.PRNGKey(9), actor, critic, K, num_minibatches=2, shuffle=True,
                                max_grad_norm=1.0, update_normalizer=True, device_rng=True)
        second = _blobs(learner)
        assert all(np.array_equal(second[k], used[k]) for k in used)
    finally:
        for h in handles:
            h.close()
        learner.close()
        env.close()
