"""The long-unroll fallback of PupperV3Env.rollout / rollout_policy / rollout_policy_sample: a
trajectory above environment.TRAJ_PINNED_MAX_BYTES lands in device buffers that are copied out after
the launch instead of in a page-locked block the launch stores into.  Both paths run the same launch,
so twin envs with the same keys must agree bit for bit: every trajectory array, the end state's
record and the returned key.  The fallback's arrays are ordinary writable arrays, the block path's
obs / reward / done read-only views.

5 envs (one half-empty wave) x 3 steps under wrap(env, episode_length=3), so the truncation rows
are not all zero; the threshold is set to 0 for the fallback run and put back in `finally`."""
import numpy as np
import pytest

from pupperv3_mjx import MODEL_XML, environment, export, rng, wrappers
from pupperv3_mjx.environment import PupperV3Env, make_keys

import common
from test_export import _brax_like_params

pytestmark = pytest.mark.gpu
N, K, D = 5, 3, 72
SHAPES = {"obs": (K, N, D), "reward": (K, N), "done": (K, N), "truncation": (K, N), "action": (K, N, 12),
          "raw_action": (K, N, 12), "log_prob": (K, N)}
KINDS = {"actions": {"obs", "reward", "done", "truncation"},
         "policy": {"obs", "reward", "done", "truncation", "action"},
         "sample": {"obs", "reward", "done", "truncation", "action", "raw_action", "log_prob"}}


def _policy(kind):
    params = _brax_like_params(np.random.RandomState(0), [72, 64, 24])
    args = ("elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12), True, 2, 30.0, 30.0)
    if kind == "sample":
        return export.DevicePolicy(export.convert_training_params(params, *args))
    return export.DevicePolicy(export.convert_params(params, *args)) if kind == "policy" else None


def _unroll(api, st, kind, dp, acts, pinned_max):
    """One unroll of `kind` with TRAJ_PINNED_MAX_BYTES = pinned_max: (state, traj, key or None)."""
    saved = environment.TRAJ_PINNED_MAX_BYTES
    try:
        environment.TRAJ_PINNED_MAX_BYTES = pinned_max
        if kind == "actions":
            return api.rollout(st, acts, truncation=True) + (None,)
        if kind == "policy":
            return api.rollout_policy(st, dp, K, truncation=True) + (None,)
        return api.rollout_policy_sample(st, dp, K, rng.PRNGKey(9), truncation=True)
    finally:
        environment.TRAJ_PINNED_MAX_BYTES = saved


def _compare(envs, apis, keys, kind, shapes):
    dp = _policy(kind)
    acts = np.random.RandomState(7).uniform(-1, 1, size=(K,) + shapes["action"][1:]).astype(np.float32)
    try:
        sb, sf = apis[0].reset(keys), apis[1].reset(keys)
        sb, block, kb = _unroll(apis[0], sb, kind, dp, acts, environment.TRAJ_PINNED_MAX_BYTES)
        sf, fall, kf = _unroll(apis[1], sf, kind, dp, acts, 0)
        assert set(block) == set(fall) == KINDS[kind]
        for k in sorted(block):
            assert block[k].shape == fall[k].shape == shapes[k], k
            assert block[k].dtype == fall[k].dtype == np.float32, k
            np.testing.assert_array_equal(block[k].view(np.uint32), fall[k].view(np.uint32), err_msg=k)
            # the fallback's arrays are the caller's own; the block path hands out views of the leased block
            assert isinstance(fall[k], np.ndarray) and fall[k].flags.writeable, k
            assert block[k].flags.writeable == (k not in ("obs", "reward", "done")), k
        np.testing.assert_array_equal(sb._record.view(np.uint32), sf._record.view(np.uint32))
        for k in ("obs", "reward", "done"):
            np.testing.assert_array_equal(np.array(getattr(sb, k)), np.array(getattr(sf, k)), err_msg=k)
        if kind == "sample":
            assert kb.dtype == kf.dtype == np.uint32 and kb.shape == kf.shape == (2,)
            np.testing.assert_array_equal(kb, kf)
            assert not np.array_equal(kb, rng.PRNGKey(9))
        assert envs[0].holds(sb) and envs[1].holds(sf)
        return block
    finally:
        if dp is not None:
            dp.close()
        for e in envs:
            e.close()


@pytest.mark.parametrize("kind", ["actions", "policy", "sample"])
def test_fallback_equals_the_block_path(require_gpu, kind):
    envs = [PupperV3Env(**common.fixture_kwargs(MODEL_XML), num_envs=N) for _ in range(2)]
    apis = [wrappers.wrap(e, episode_length=3) for e in envs]
    block = _compare(envs, apis, make_keys(2, N), kind, SHAPES)
    assert (block["truncation"] == 1).sum() >= 1  # episode_length = K: the rows are not all zero
    assert np.all(block["done"][block["truncation"] == 1] == 1)


def test_fallback_equals_the_block_path_single_env_state(require_gpu):
    """rollout() from a single-env state (one key [2]): the trajectories lose the env axis on both paths."""
    envs = [PupperV3Env(**common.fixture_kwargs(MODEL_XML), num_envs=1) for _ in range(2)]
    apis = [wrappers.wrap(e, episode_length=3) for e in envs]
    shapes = {k: (K,) + s[2:] for k, s in SHAPES.items()}
    block = _compare(envs, apis, make_keys(2, 1)[0], "actions", shapes)
    assert block["truncation"][K - 1] == 1
