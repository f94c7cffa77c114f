"""Network initialisation and the checkpoint file without a device: ppo.init_params (the numpy
restatement of pp3_learner_init_params: its range, variance, zero biases and key schedule, in both
jax_threefry_partitionable layouts), the entry point's binding and null-argument refusals, and
ppo.save_checkpoint / load_checkpoint on hand-built dicts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pupperv3_mjx import _lib, export, ppo, rng

F, U = np.float32, np.uint32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pupper_hip.h")
FAN_IN, WIDTH = 72, 256


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


@pytest.mark.parametrize("part", [True, False], ids=["partitionable", "legacy"])
def test_init_params_range_variance_and_zero_biases(part):
    """72 -> 256 -> 256 -> 24: every kernel entry in [-s, s) with s = sqrt(3 / fan_in) in f32, biases
    exactly 0, and for the 72 x 256 kernel the sample variance within 5 % of 1 / fan_in.  The bound
    is derived, not measured: the variance of U(-s, s) is s^2 / 3 = 1 / fan_in, and the sample variance
    of n uniform draws has relative standard deviation sqrt((kurtosis - 1) / n) = sqrt(0.8 / n); at
    n = 72 * 256 = 18432 that is 0.66 %, so 5 % is more than 7 standard deviations."""
    layers = ppo.init_params(rng.PRNGKey(7), FAN_IN, (WIDTH, WIDTH), 24, part)
    assert [k.shape for k, _ in layers] == [(FAN_IN, WIDTH), (WIDTH, WIDTH), (WIDTH, 24)]
    fan_in = FAN_IN
    for k, b in layers:
        s = np.sqrt(F(3.0) * (F(1.0) / F(fan_in)))
        assert k.dtype == F and b.dtype == F and s.dtype == F
        assert np.all(k >= -s) and np.all(k < s)
        assert b.shape == (k.shape[1],) and not _bits(b).any()
        fan_in = k.shape[1]
    k0 = layers[0][0].astype(np.float64)
    n = k0.size
    assert n == 18432 and np.sqrt(0.8 / n) < 0.05 / 7
    var = np.mean((k0 - k0.mean()) ** 2)
    assert abs(var * FAN_IN - 1.0) < 0.05, var * FAN_IN


@pytest.mark.parametrize("part", [True, False], ids=["partitionable", "legacy"])
def test_key_schedule_is_the_documented_chain_of_two_way_splits(part):
    """k_net, k_l = split(k_net) per layer in order, the kernel uniform(k_l, (fan_in, out), -1, 1) * s:
    written out by hand for 72 -> 5 -> 3 -> 24 (5 x 3: an odd count, the legacy layout's padded one)."""
    key = np.array([0x1234, 0xABCD], U)
    got = ppo.init_params(key, FAN_IN, (5, 3), 24, part)
    k1, ka = rng.split(key, 2, part)
    k2, kb = rng.split(k1, 2, part)
    _, kc = rng.split(k2, 2, part)
    for (k, b), kl, (fi, m) in zip(got, (ka, kb, kc), ((72, 5), (5, 3), (3, 24))):
        s = np.sqrt(F(3.0) * (F(1.0) / F(fi)))
        want = rng.uniform(kl, (fi, m), -1.0, 1.0, part) * s
        assert want.dtype == F
        np.testing.assert_array_equal(_bits(k), _bits(want))
        assert b.shape == (m,)
    # the other layout draws other bits
    other = ppo.init_params(key, FAN_IN, (5, 3), 24, not part)
    assert all(np.any(a[0] != o[0]) for a, o in zip(got, other))


@pytest.mark.parametrize("part", [True, False], ids=["partitionable", "legacy"])
def test_layers_and_nets_draw_from_distinct_keys(part):
    """Equal shapes inside a net (256 x 256 twice) and across the two nets of a learner key
    (k_policy, k_value = split(key)): no two kernels of equal shape are equal."""
    k_policy, k_value = rng.split(rng.PRNGKey(3), 2, part)
    assert np.any(k_policy != k_value)
    pol = ppo.init_params(k_policy, FAN_IN, (WIDTH, WIDTH, WIDTH), 24, part)
    val = ppo.init_params(k_value, FAN_IN, (WIDTH, WIDTH, WIDTH), 1, part)
    kernels = [k for k, _ in pol + val]
    pairs = 0
    for i in range(len(kernels)):
        for j in range(i + 1, len(kernels)):
            if kernels[i].shape == kernels[j].shape:
                pairs += 1
                assert np.mean(kernels[i] == kernels[j]) < 0.01, (i, j)
    assert pairs == 1 + 6  # the two 72 x 256, and the four 256 x 256 among themselves
    # the same key again: the same bits
    again = ppo.init_params(k_policy, FAN_IN, (WIDTH, WIDTH, WIDTH), 24, part)
    assert all(np.array_equal(_bits(a[0]), _bits(b[0])) for a, b in zip(pol, again))


def test_entry_point_is_exported_declared_bound_and_refuses_nulls():
    L = _lib.load()
    name = "pp3_learner_init_params"
    assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"^int %s\(" % name, open(HEADER).read(), re.M)
    assert L.pp3_learner_init_params.argtypes is not None and L.pp3_learner_init_params.restype is C.c_int
    key = (C.c_uint32 * 2)(0, 1)
    for args in ((None, key, 1, None), (C.c_void_p(16), None, 1, None), (None, None, 0, None)):
        assert L.pp3_learner_init_params(*args) == 1  # PP3_ERR_ARG, before any GPU work
        assert b"pp3_learner_init_params" in L.pp3_learn_last_error()


def test_zero_network_dicts_have_the_learner_shapes():
    meta = dict(action_scale=0.75, kp=5.0, kd=0.25, default_pose=np.zeros(12), joint_upper_limits=np.ones(12),
                joint_lower_limits=-np.ones(12), use_imu=True, observation_history=2, maximum_pitch_command=30.0,
                maximum_roll_command=30.0)
    pol, val = export.zero_network_dicts(72, (5, 3), (7,), "elu", 0.01, 2.0, **meta)
    assert export.layers_blob(pol)[1].tolist() == [5, 3, 24] and export.layers_blob(val)[1].tolist() == [7, 1]
    assert export.layers_blob(pol)[2].tolist() == [2, 2, 0] and export.layers_blob(val)[2].tolist() == [2, 0]
    assert not export.layers_blob(pol)[3].any() and export.layers_blob(pol)[3].size == 73 * 5 + 6 * 3 + 4 * 24
    assert pol["distribution"] == {"type": "normal_tanh", "min_std": 0.01, "var_scale": 2.0}
    assert pol["action_scale"] == 0.75 and pol["observation_history"] == 2 and val["observation_history"] == 2
    bare, _ = export.zero_network_dicts(72, (5,), (7,))
    assert set(bare) == {"in_shape", "layers", "distribution"}
    with pytest.raises(ValueError, match="metadata"):
        export.zero_network_dicts(72, (5,), (7,), kp=5.0)


# ------------------------------------------------------------------------------ the checkpoint file
def _parts(seed):
    rs = np.random.RandomState(seed)
    payload = rs.normal(size=37).astype(F)
    pb = payload.view(U)
    pb[3], pb[4], pb[5] = 0x7FC00001, 0xFFC12345, 0x7F800001  # quiet and signalling NaN patterns
    pb[6], pb[7] = 0x80000000, 0x00000001                      # -0, the smallest denormal
    learner = {"policy_params": payload, "t": np.asarray(8, np.int64), "min_std": np.asarray(0.001, F),
               "running_statistics": np.asarray(True), "policy_widths": np.array([16, 24], np.int32)}
    env = {"field_0": rs.randint(0, 2 ** 32, size=(6, 11), dtype=np.uint64).astype(U), "layout_num_envs": np.asarray(6, np.int64)}
    ev = {"key": np.array([0xFFFFFFFF, 0x80000001], U)}
    loop = {"k_train": np.array([0xDEADBEEF, 7], U), "iteration": np.asarray(2, np.int64),
            "walltime": np.asarray(1.25, np.float64), "schedule_eval_steps": np.array([0, 36, 72], np.int64)}
    return dict(learner=learner, env=env, evaluator=ev, loop=loop)


def _assert_same(got, want):
    assert set(got) == set(want)
    for part in want:
        assert set(got[part]) == set(want[part]), part
        for k, v in want[part].items():
            g = got[part][k]
            assert g.dtype == v.dtype and g.shape == v.shape, (part, k)
            assert g.tobytes() == np.ascontiguousarray(v).tobytes(), (part, k)


def test_checkpoint_round_trip_is_bit_equal_and_atomic(tmp_path):
    path = tmp_path / "ck.npz"
    p = _parts(0)
    ppo.save_checkpoint(path, p["learner"], p["env"], None, p["evaluator"], p["loop"])
    assert sorted(os.listdir(tmp_path)) == ["ck.npz"]  # no temporary file left behind
    with np.load(path, allow_pickle=False) as z:       # plain arrays only
        assert "learner/policy_params" in z.files and z["loop/k_train"].dtype == U and z["learner/t"].shape == ()
    _assert_same(ppo.load_checkpoint(path), p)
    # an existing file at the path is replaced whole: other arrays, and a part fewer
    q = _parts(1)
    del q["evaluator"]
    q["learner"].pop("policy_widths")
    ppo.save_checkpoint(str(path), q["learner"], q["env"], loop=q["loop"])
    assert sorted(os.listdir(tmp_path)) == ["ck.npz"]
    _assert_same(ppo.load_checkpoint(str(path)), q)


def test_checkpoint_refuses_objects_and_leaves_the_old_file(tmp_path):
    path = tmp_path / "ck.npz"
    p = _parts(2)
    ppo.save_checkpoint(path, p["learner"], p["env"])
    before = path.read_bytes()
    with pytest.raises(ValueError, match="plain arrays"):
        ppo.save_checkpoint(path, dict(p["learner"], extra=np.array([{"a": 1}], dtype=object)), p["env"])
    assert path.read_bytes() == before and sorted(os.listdir(tmp_path)) == ["ck.npz"]
    other = tmp_path / "other.npz"
    np.savez(other, a=np.zeros(3))
    with pytest.raises(ValueError, match="not a checkpoint"):
        ppo.load_checkpoint(other)
