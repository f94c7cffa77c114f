"""Policy export in the reference's deployment format (export.py:7-81) and its device runner.

`convert_params` restates export.py:13-81 in numpy (the reference imports jax only for
`jp.split`): observation normalisation folded into the first dense layer
(`fold_in_normalization`, export.py:7-10), the final layer cut to its first half (the mean of
Brax PPO's tanh-Gaussian head), per-layer activation names from utils.activation_fn_map
(relu, sigmoid, elu, tanh), metadata keys as in export.py:63-79.  `policy_forward` is the numpy
meaning of that JSON (what the robot runs); `DevicePolicy` runs it batched on the GPU
(csrc/pp3_policy.hip, f32 matrix cores) straight from the env's observation buffer, so a
policy + env rollout never leaves the device.

`convert_training_params` is the training form of the same network: the whole Gaussian head (24
linear columns) plus the distribution's constants, which is what Brax PPO collects data with
([ext] brax 0.12.1 training/distribution.py NormalTanhDistribution; quoted from memory, Brax is
not vendored in the reference).  `sample_forward` is its float64 numpy meaning and
`DevicePolicy.sample` / `sample_env` / `PupperV3Env.rollout_policy_sample` run it on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Mapping

import numpy as np

ACTIVATIONS = {"linear": 0, "relu": 1, "elu": 2, "tanh": 3, "sigmoid": 4}


def fold_in_normalization(A, b, mean, std):
    """export.py:7-10: dense(x_norm) with x_norm = (x - mean) / std  ==  dense'(x)."""
    A = np.asarray(A)
    b = np.asarray(b)
    mean = np.asarray(mean)
    std = np.asarray(std)
    A_prime = A / std[:, np.newaxis]
    b_prime = (b - (A.T @ (mean / std)[:, np.newaxis]).T)[0]
    return A_prime, b_prime


def _field(obj, name):
    return obj[name] if isinstance(obj, Mapping) else getattr(obj, name)


def convert_params(params, activation: str, action_scale: float, kp: float, kd: float, default_pose,
                   joint_upper_limits, joint_lower_limits, use_imu: bool, observation_history: int,
                   maximum_pitch_command: float, maximum_roll_command: float,
                   final_activation: str = "tanh") -> Dict[str, Any]:
    """export.py:13-81.  params = (normalizer with .mean/.std, {"params": {layer: {"kernel", "bias"}}})."""
    layers, input_size = _dense_layers(params, activation, final_activation, split_head=True)
    return _policy_dict(layers, input_size, action_scale, kp, kd, default_pose, joint_upper_limits,
                        joint_lower_limits, use_imu, observation_history, maximum_pitch_command,
                        maximum_roll_command)


def _dense_layers(params, activation: str, final_activation: str, split_head: bool):
    """export.py:25-58: the dense layers of the exported JSON; split_head cuts the final layer to
    its first half (the Gaussian head's mean) as the deployment export does."""
    mean, std = _field(params[0], "mean"), _field(params[0], "std")
    params_dict = params[1]["params"]
    layers = []
    input_size = None
    for i, (layer_name, layer_params) in enumerate(params_dict.items()):
        is_first_layer = i == 0
        is_final_layer = i == len(params_dict) - 1
        bias = np.asarray(layer_params["bias"])
        kernel = np.asarray(layer_params["kernel"])
        if is_first_layer:
            kernel, bias = fold_in_normalization(A=kernel, b=bias, mean=mean, std=std)
            input_size = kernel.shape[0]
        if is_final_layer and split_head:
            bias, _ = np.split(bias, 2, axis=-1)
            kernel, _ = np.split(kernel, 2, axis=-1)
        layers.append({
            "type": "dense",
            "activation": activation if not is_final_layer else final_activation,
            "shape": [None, len(bias)],
            "weights": [kernel.tolist(), bias.tolist()],
        })
    return layers, input_size


def _policy_dict(layers, input_size, action_scale, kp, kd, default_pose, joint_upper_limits, joint_lower_limits,
                 use_imu, observation_history, maximum_pitch_command, maximum_roll_command) -> Dict[str, Any]:
    return {
        "use_imu": use_imu,
        "control_orientation": True,
        "observation_history": observation_history,
        "action_scale": action_scale,
        "kp": kp,
        "kd": kd,
        "default_joint_pos": np.array(default_pose).tolist(),
        "joint_upper_limits": np.array(joint_upper_limits).tolist(),
        "joint_lower_limits": np.array(joint_lower_limits).tolist(),
        "maximum_pitch_command": maximum_pitch_command,
        "maximum_roll_command": maximum_roll_command,
        "in_shape": [None, input_size],
        "layers": layers,
    }


def _act_np(x, name):
    name = name.lower()
    if name == "relu":
        return np.maximum(x, 0)
    if name == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    if name == "tanh":
        return np.tanh(x)
    if name == "sigmoid":
        return 1 / (1 + np.exp(-x))
    if name == "linear":
        return x
    raise ValueError(f"unsupported activation {name!r}")


def policy_forward(policy: Dict[str, Any], obs) -> np.ndarray:
    """Reference meaning of a converted policy: h = act(h @ kernel + bias) per layer."""
    h = np.asarray(obs, dtype=np.float64)
    for layer in policy["layers"]:
        k, b = layer["weights"]
        h = _act_np(h @ np.asarray(k, dtype=np.float64) + np.asarray(b, dtype=np.float64), layer["activation"])
    return h


def convert_training_params(params, activation: str, action_scale: float, kp: float, kd: float, default_pose,
                            joint_upper_limits, joint_lower_limits, use_imu: bool, observation_history: int,
                            maximum_pitch_command: float, maximum_roll_command: float,
                            min_std: float = 0.001, var_scale: float = 1.0) -> Dict[str, Any]:
    """The training form of `convert_params` (same inputs): the final layer keeps all 24 columns
    (12 means, 12 pre-softplus scales) with "linear" activation, and "distribution" names Brax
    PPO's NormalTanhDistribution with its constants (Brax's defaults, quoted from memory).
    tanh of the first 12 outputs is what `convert_params` exports."""
    layers, input_size = _dense_layers(params, activation, "linear", split_head=False)
    out = _policy_dict(layers, input_size, action_scale, kp, kd, default_pose, joint_upper_limits,
                       joint_lower_limits, use_imu, observation_history, maximum_pitch_command,
                       maximum_roll_command)
    out["distribution"] = {"type": "normal_tanh", "min_std": float(min_std), "var_scale": float(var_scale)}
    return out


def convert_value_params(params, activation: str, observation_history: int) -> Dict[str, Any]:
    """Brax PPO's value network ([ext] brax 0.12.1 training/agents/ppo/networks.py make_value_network:
    an MLP on the normalised observation whose last layer has one column; from memory) in the
    dict form of `convert_params`: params = (normalizer with .mean/.std, {"params": {layer:
    {"kernel", "bias"}}}), normalisation folded into layer 0, hidden layers `activation`, the last
    layer "linear" with shape [None, 1].  It has no actuator keys and no distribution:
    `policy_forward` is its meaning and `DevicePolicy.act` with action_stride 1 runs it (the critic
    of `PupperV3Env.collect_ppo`)."""
    layers, input_size = _dense_layers(params, activation, final_activation="linear", split_head=False)
    if layers[-1]["shape"][1] != 1:
        raise ValueError(f"a value network's last layer has one column, this one has {layers[-1]['shape'][1]}")
    return {"observation_history": observation_history, "in_shape": [None, input_size], "layers": layers}


METADATA_KEYS = ("action_scale", "kp", "kd", "default_pose", "joint_upper_limits", "joint_lower_limits", "use_imu",
                 "observation_history", "maximum_pitch_command", "maximum_roll_command")


def zero_network_dicts(observation_size: int, policy_hidden_layer_sizes, value_hidden_layer_sizes,
                       activation: str = "elu", min_std: float = 0.001, var_scale: float = 1.0, **metadata):
    """(policy dict, value dict) in the forms of `convert_training_params` and `convert_value_params`
    for Brax's make_ppo_networks shapes, un-folded and with all-zero f32 weights: the policy
    observation_size -> hidden.. -> 24 (the normal_tanh head), the value net observation_size ->
    hidden.. -> 1, hidden layers `activation`, last layers linear.  For ppo.make_learner, which
    fills the weights on the device.  `metadata`: none, or all of METADATA_KEYS (convert_params'
    arguments of those names: what the deployment JSON carries beside "layers")."""
    if activation.lower() not in ACTIVATIONS:
        raise ValueError(f"unsupported activation {activation!r} (device: {sorted(ACTIVATIONS)})")
    if metadata and set(metadata) != set(METADATA_KEYS):
        raise ValueError(f"the export metadata is none or all of {METADATA_KEYS}; got {sorted(metadata)}")

    def layers(widths):
        out, k = [], int(observation_size)
        for i, m in enumerate(widths):
            out.append({"type": "dense", "activation": activation if i < len(widths) - 1 else "linear",
                        "shape": [None, int(m)],
                        "weights": [np.zeros((k, int(m)), np.float32), np.zeros(int(m), np.float32)]})
            k = int(m)
        return out

    pl = layers(tuple(policy_hidden_layer_sizes) + (24,))
    if metadata:
        policy = _policy_dict(pl, int(observation_size), *(metadata[k] for k in METADATA_KEYS))
    else:
        policy = {"in_shape": [None, int(observation_size)], "layers": pl}
    policy["distribution"] = {"type": "normal_tanh", "min_std": float(min_std), "var_scale": float(var_scale)}
    value = {"in_shape": [None, int(observation_size)], "layers": layers(tuple(value_hidden_layer_sizes) + (1,))}
    if "observation_history" in metadata:
        value["observation_history"] = metadata["observation_history"]
    return policy, value


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def normal_tanh_scale(logits, min_std: float = 0.001, var_scale: float = 1.0):
    """(loc, scale) of the head: loc = logits[..., :12], scale = (softplus(logits[..., 12:]) + min_std) * var_scale."""
    logits = np.asarray(logits, dtype=np.float64)
    loc, s = np.split(logits, 2, axis=-1)
    return loc, (_softplus(s) + min_std) * var_scale


def normal_tanh_log_prob(logits, raw, min_std: float = 0.001, var_scale: float = 1.0) -> np.ndarray:
    """Brax's NormalTanhDistribution.log_prob(logits, raw_action), float64: the normal's log
    density of raw minus the tanh's log Jacobian in its stable form 2 (log 2 - raw - softplus(-2 raw))
    (log(1 - tanh(raw)^2) underflows to log(0) from |raw| ~ 19), summed over the 12 actions."""
    loc, scale = normal_tanh_scale(logits, min_std, var_scale)
    raw = np.asarray(raw, dtype=np.float64)
    zr = (raw - loc) / scale
    terms = (-0.5 * zr * zr - np.log(scale) - 0.5 * np.log(2 * np.pi)
             - 2.0 * (np.log(2.0) - raw - _softplus(-2.0 * raw)))
    return terms.sum(axis=-1)


def sample_forward(policy: Dict[str, Any], obs, key, partitionable: bool = True):
    """Float64 numpy meaning of a training policy's sample: `obs` [n, in] -> (action [n, 12],
    raw [n, 12], log_prob [n], logits [n, 24]) with the noise rng.normal(key, (n, 12)): row i,
    column j takes element i * 12 + j of the key's stream."""
    from . import rng
    dist = policy["distribution"]
    if dist["type"] != "normal_tanh":
        raise ValueError(f"unsupported distribution {dist['type']!r}")
    logits = policy_forward(policy, np.atleast_2d(np.asarray(obs, dtype=np.float64)))
    loc, scale = normal_tanh_scale(logits, dist["min_std"], dist["var_scale"])
    z = rng.normal(key, loc.shape, partitionable).astype(np.float64)
    raw = loc + scale * z
    return np.tanh(raw), raw, normal_tanh_log_prob(logits, raw, dist["min_std"], dist["var_scale"]), logits


def layers_blob(policy: Dict[str, Any]):
    """(in_dim, out_dims int32[], activations int32[], f32 blob) of a converted dict's layers: the
    arguments of pp3_policy_create (blob = per layer kernel [in][out] row-major, then bias [out])."""
    in_dim = int(policy["in_shape"][1])
    outs, acts, blob = [], [], []
    k_in = in_dim
    for layer in policy["layers"]:
        k, b = np.asarray(layer["weights"][0], dtype=np.float32), np.asarray(layer["weights"][1], dtype=np.float32)
        if k.shape != (k_in, b.shape[0]):
            raise ValueError(f"layer kernel {k.shape} does not follow input width {k_in}")
        name = layer["activation"].lower()
        if name not in ACTIVATIONS:
            raise ValueError(f"unsupported activation {name!r} (device: {sorted(ACTIVATIONS)})")
        outs.append(b.shape[0])
        acts.append(ACTIVATIONS[name])
        blob += [k.ravel(), b]
        k_in = b.shape[0]
    return (in_dim, np.array(outs, dtype=np.int32), np.array(acts, dtype=np.int32),
            np.ascontiguousarray(np.concatenate(blob), dtype=np.float32))


DIST_NORMAL_TANH = 1  # PP3_DIST_NORMAL_TANH


class DevicePolicy:
    """Batched on-device forward of a converted policy dict (pp3_policy_* C ABI).  A dict from
    `convert_training_params` (with "distribution") also samples: `sample`, `sample_env`."""

    def __init__(self, policy: Dict[str, Any], device: int = 0):
        from . import _lib
        self._lib = _lib
        L = _lib.load()
        self._L = L
        in_dim, o, a, w = layers_blob(policy)
        h = C.c_void_p()
        _lib.check(L.pp3_policy_create(int(device), in_dim, len(o), o.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                       w.ctypes.data_as(C.c_void_p), C.byref(h)), "policy")
        self._h = h
        self.in_dim = in_dim
        self.out_dim = int(o[-1])
        self.device = int(device)
        self.distribution = None
        dist = policy.get("distribution")
        if dist is not None:
            if dist.get("type") != "normal_tanh":
                self.close()
                raise ValueError(f"unsupported distribution {dist.get('type')!r} (device: 'normal_tanh')")
            try:
                _lib.check(L.pp3_policy_set_distribution(h, DIST_NORMAL_TANH, float(dist["min_std"]),
                                                         float(dist["var_scale"])), "policy")
            except _lib.PupperHipError:
                self.close()
                raise
            self.distribution = dict(dist)

    def act(self, obs_dev: int, obs_stride: int, n: int, actions_dev: int, action_stride: int, stream=None) -> None:
        self._lib.check(self._L.pp3_policy_act(
            self._h, C.c_void_p(obs_dev), int(obs_stride), int(n), C.c_void_p(actions_dev), int(action_stride),
            C.c_void_p(stream) if stream else None), "policy")

    def act_env(self, env, actions_dev: int, stream=None) -> None:
        """actions[N][12] = policy(env's current observation buffer)."""
        from . import _abi
        if self.out_dim != _abi.NU:
            raise ValueError(f"act_env needs a policy with {_abi.NU} outputs (the action), this one has {self.out_dim}")
        obs_ptr, obs_n = env.device_field(_abi.F_OBS)
        if stream is None:  # order with the env's kernels
            stream = env._L.pp3_stream(env._h)
        self.act(obs_ptr, obs_n, env.num_envs, actions_dev, _abi.NU, stream)

    def sample(self, obs_dev: int, obs_stride: int, n: int, key, actions_dev: int, action_stride: int,
               raw_dev: int = 0, logp_dev: int = 0, logits_dev: int = 0, partitionable: bool = True, stream=None) -> None:
        """One tanh-Gaussian sample per row from `key` (uint32[2]): actions [n][12] (row stride
        action_stride) = tanh(raw); raw [n][12], log_prob [n] and logits [n][24] where given."""
        k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
        p = lambda v: C.c_void_p(v) if v else None
        self._lib.check(self._L.pp3_policy_sample(
            self._h, C.c_void_p(obs_dev), int(obs_stride), int(n), k.ctypes.data_as(C.c_void_p), int(bool(partitionable)),
            C.c_void_p(actions_dev), int(action_stride), p(raw_dev), p(logp_dev), p(logits_dev),
            C.c_void_p(stream) if stream else None), "policy")

    def sample_env(self, env, key, actions_dev: int, raw_dev: int = 0, logp_dev: int = 0, logits_dev: int = 0,
                   stream=None) -> None:
        """actions[N][12] ~ policy(env's current observation buffer), with the env's rng_partitionable."""
        from . import _abi
        obs_ptr, obs_n = env.device_field(_abi.F_OBS)
        if stream is None:  # order with the env's kernels
            stream = env._L.pp3_stream(env._h)
        self.sample(obs_ptr, obs_n, env.num_envs, key, actions_dev, _abi.NU, raw_dev, logp_dev, logits_dev,
                    env._partitionable, stream)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.pp3_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
