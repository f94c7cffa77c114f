"""Brax PPO's learner step on the device (csrc/pp3_learn.hip; the contract is the comment above
pp3_learner_create in include/pupper_hip.h): compute_ppo_loss's gradients for both networks on a
minibatch of a `PupperV3Env.collect_ppo` batch, Adam, and the reload of the actor and critic
handles from the trained parameters, all on the env's stream without a host round trip.

    learner = PPOLearner(policy_dict, value_dict, normalizer=(mean, std))
    actor, critic = learner.make_policies()
    state, metrics, key = learner.train_iteration(env, state, key, actor, critic, nsteps=20)

Not here (follow-ups): the running-statistics update of the normaliser, shuffled minibatches (an
index gather; minibatches are contiguous env ranges), gradient clipping and learning-rate
schedules, bf16 / mixed precision, the multi-GPU gradient all-reduce.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _abi, _lib, rng
from .export import DevicePolicy, layers_blob

ROW_CHUNK = 256  # PP3_LEARN_ROW_CHUNK: rows per partial sum of the weight gradient
METRICS = ("total_loss", "policy_loss", "v_loss", "entropy_loss")
HPARAMS = dict(discount=0.97, gae_lambda=0.95, reward_scaling=1.0, clipping_epsilon=0.3, entropy_cost=1e-2,
               normalize_advantage=True)


def _base(env):
    """The PupperV3Env behind `env` (itself, or the one a wrappers.wrap episode wrapper drives)."""
    return getattr(env, "env", env)


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class PPOLearner:
    """Trainable copies of a policy (`export.convert_training_params`) and a value network
    (`export.convert_value_params`) whose layers were converted UN-folded (a normaliser of mean 0
    and std 1), plus the normaliser itself (`normalizer` = (mean, std) or an object with .mean and
    .std; None: identity), held on the device with their gradients and Adam moments."""

    def __init__(self, policy_dict: Dict[str, Any], value_dict: Dict[str, Any], normalizer=None, device: int = 0,
                 max_rows: int = 21 * 4096):
        L = _lib.load()
        self._L = L
        dist = policy_dict.get("distribution")
        if dist is None or dist.get("type") != "normal_tanh":
            raise ValueError("the policy needs the 'normal_tanh' distribution (export.convert_training_params)")
        self._dicts = (policy_dict, value_dict)
        pin, pout, pact, pblob = layers_blob(policy_dict)
        vin, vout, vact, vblob = layers_blob(value_dict)
        if pin != vin:
            raise ValueError(f"policy and value network read different observations ({pin} and {vin} inputs)")
        self.in_dim, self.device, self.max_rows = pin, int(device), int(max_rows)
        self._shapes = ((pin, pout, pact), (vin, vout, vact))
        self.distribution = dict(dist)
        h = C.c_void_p()
        rc = L.pp3_learner_create(self.device, pin, len(pout), _vp(pout), _vp(pact), _vp(pblob), len(vout), _vp(vout),
                                  _vp(vact), _vp(vblob), float(dist["min_std"]), float(dist["var_scale"]),
                                  self.max_rows, C.byref(h))
        if rc != 0:
            raise _lib.PupperHipError(L.pp3_learn_last_error().decode())
        self._h = h
        self._norm = None
        if normalizer is not None:
            mean, std = (normalizer if isinstance(normalizer, (tuple, list))
                         else (normalizer.mean, normalizer.std))
            ms = np.ascontiguousarray(np.stack([np.asarray(mean, np.float32), np.asarray(std, np.float32)]))
            if ms.shape != (2, pin):
                raise ValueError(f"the normaliser needs mean and std of {pin} entries")
            self._norm = _lib.DeviceBuffer(ms.nbytes, self.device)
            self._norm.upload(ms)
        self._metrics = _lib.DeviceBuffer(16, self.device)
        self._eps = None  # (key bytes, shape, DeviceBuffer)
        self._env = None  # the env whose stream the last call ran on
        self.t = 0        # Adam steps taken

    # ---- device views -------------------------------------------------------------------------
    def buffer(self, net: int, which: int) -> Tuple[int, int]:
        """(device address, element count): net 0 policy / 1 value; which 0 parameters, 1 gradients, 2 m, 3 v."""
        p, n = C.c_void_p(), C.c_int64()
        self._check(self._L.pp3_learner_buffers(self._h, int(net), int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    def _norm_ptrs(self):
        if self._norm is None:
            return None, None
        return C.c_void_p(self._norm.ptr.value), C.c_void_p(self._norm.ptr.value + 4 * self.in_dim)

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise _lib.PupperHipError(f"pupper_hip error {rc}: {self._L.pp3_learn_last_error().decode(errors='replace')}")

    def _wait(self) -> None:
        if self._env is not None:
            self._env.synchronize()

    def _download(self, net: int, which: int) -> np.ndarray:
        self._wait()
        ptr, n = self.buffer(net, which)
        out = np.empty(n, np.float32)
        _lib.check(self._L.pp3_memcpy_d2h(_vp(out), C.c_void_p(ptr), out.nbytes))
        return out

    def _layers(self, net: int, flat: np.ndarray) -> List[Tuple[np.ndarray, np.ndarray]]:
        in_dim, outs, _ = self._shapes[net]
        res, off, k = [], 0, in_dim
        for m in outs:
            m = int(m)
            res.append((flat[off:off + k * m].reshape(k, m), flat[off + k * m:off + (k + 1) * m]))
            off += (k + 1) * m
            k = m
        return res

    def params(self) -> Dict[str, List[Tuple[np.ndarray, np.ndarray]]]:
        """{"policy" | "value": [(kernel [in][out], bias [out]) per layer]} downloaded (checkpoints, tests)."""
        return {"policy": self._layers(0, self._download(0, 0)), "value": self._layers(1, self._download(1, 0))}

    def grads(self) -> Dict[str, List[Tuple[np.ndarray, np.ndarray]]]:
        return {"policy": self._layers(0, self._download(0, 1)), "value": self._layers(1, self._download(1, 1))}

    def metrics(self) -> Dict[str, float]:
        """The last loss_and_grad's total / policy / value / entropy losses (waits for it)."""
        self._wait()
        out = np.empty(4, np.float32)
        self._metrics.download(out)
        return dict(zip(METRICS, (float(x) for x in out)))

    # ---- the step -----------------------------------------------------------------------------
    def loss_and_grad_device(self, K: int, B: int, N: int, e0: int, obs_all: int, raw_action: int, log_prob: int,
                             reward: int, done: int, truncation: int, eps: int, stream=None, discount: float = 0.97,
                             gae_lambda: float = 0.95, reward_scaling: float = 1.0, clipping_epsilon: float = 0.3,
                             entropy_cost: float = 1e-2, normalize_advantage: bool = True) -> None:
        """pp3_ppo_loss_grad on device addresses (arrays of a batch of N envs and K steps, see the header)."""
        p = lambda v: C.c_void_p(v) if v else None
        mean, std = self._norm_ptrs()
        self._check(self._L.pp3_ppo_loss_grad(
            self._h, int(K), int(B), int(N), int(e0), p(obs_all), p(raw_action), p(log_prob), p(reward), p(done),
            p(truncation), p(eps), mean, std, float(discount), float(gae_lambda), float(reward_scaling),
            float(clipping_epsilon), float(entropy_cost), int(bool(normalize_advantage)), self._metrics.ptr,
            p(stream)))

    def _eps_for(self, env, eps_key, shape) -> int:
        """The entropy noise rng.normal(eps_key, [K][N][12]) on the device: drawn on the host and
        uploaded once per key (one upload per iteration, shared by its minibatches)."""
        k = np.asarray(eps_key, dtype=np.uint32).reshape(2)
        tag = (k.tobytes(), tuple(shape))
        if self._eps is None or self._eps[0] != tag:
            z = rng.normal(k, shape, env._partitionable)
            if self._eps is not None:
                self._eps[1].free()
            buf = _lib.DeviceBuffer(z.nbytes, self.device)
            buf.upload(z)
            self._eps = (tag, buf)
        return self._eps[1].ptr.value

    def loss_and_grad(self, env, e0: int, B: int, eps_key, **hparams) -> None:
        """Loss and gradients on envs [e0, e0 + B) of the env's last collect_ppo batch, on the env's
        stream.  hparams: HPARAMS' keys.  Results: grads(), metrics()."""
        dev = env.ppo_device_batch()
        ptr, (K, N, D) = dev["observation"]
        if D != self.in_dim:
            raise ValueError(f"the batch's observations have {D} entries, the networks read {self.in_dim}")
        env = _base(env)
        eps = self._eps_for(env, eps_key, (K, N, _abi.NU))
        self._env = env
        self.loss_and_grad_device(K, B, N, e0, ptr, dev["raw_action"][0], dev["log_prob"][0], dev["reward"][0],
                                  dev["done"][0], dev["truncation"][0], eps, env._L.pp3_stream(env._h),
                                  **{**HPARAMS, **hparams})

    def adam_step(self, lr: float, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, stream=None) -> None:
        """optax.adam's update of both nets from the gradients of the last loss_and_grad.  stream: by
        default the stream of the env the last loss_and_grad read (else the default stream)."""
        if stream is None and self._env is not None:
            stream = self._env._L.pp3_stream(self._env._h)
        t = self.t + 1
        c1, c2 = np.float32(1.0 - float(b1) ** t), np.float32(1.0 - float(b2) ** t)
        self._check(self._L.pp3_adam_step(self._h, float(lr), float(b1), float(b2), float(eps), float(c1), float(c2),
                                          C.c_void_p(stream) if stream else None))
        self.t = t

    def make_policies(self) -> Tuple[DevicePolicy, DevicePolicy]:
        """(actor, critic) handles of the networks' shapes, loaded with the current parameters."""
        actor, critic = DevicePolicy(self._dicts[0], self.device), DevicePolicy(self._dicts[1], self.device)
        self.sync(actor, critic)
        return actor, critic

    def sync(self, device_policy: Optional[DevicePolicy], device_value: Optional[DevicePolicy], stream=None) -> None:
        """Reloads the handles (either may be None) from the current parameters, the normaliser
        folded into layer 0 (pp3_policy_load_params)."""
        if stream is None and self._env is not None:
            stream = self._env._L.pp3_stream(self._env._h)
        mean, std = self._norm_ptrs()
        for net, pol in ((0, device_policy), (1, device_value)):
            if pol is None:
                continue
            in_dim, outs, _ = self._shapes[net]
            self._check(self._L.pp3_policy_load_params(pol._h, C.c_void_p(self.buffer(net, 0)[0]), in_dim, len(outs),
                                                       _vp(outs), mean, std, C.c_void_p(stream) if stream else None))

    def train_iteration(self, env, state, key, device_policy: DevicePolicy, device_value: DevicePolicy, nsteps: int,
                        num_minibatches: int = 1, num_updates_per_batch: int = 1, lr: float = 3e-4, **hparams):
        """One PPO iteration: collect_ppo with the handles, num_updates_per_batch passes over
        num_minibatches contiguous env ranges (loss, gradient, Adam each), then the reload.
        key -> (collect key, entropy-noise key) by rng.split.  Returns (state, metrics of the last
        minibatch, the collect's key chain end)."""
        base = _base(env)
        n = base.num_envs
        if n % num_minibatches:
            raise ValueError(f"{n} envs do not divide into {num_minibatches} minibatches")
        B = n // num_minibatches
        k_collect, k_eps = rng.split(np.asarray(key, dtype=np.uint32).reshape(2), 2, base._partitionable)
        gae = {k: hparams[k] for k in ("discount", "gae_lambda", "reward_scaling") if k in hparams}
        state, _, k_out = env.collect_ppo(state, device_policy, device_value, nsteps, k_collect, **gae)
        for _ in range(num_updates_per_batch):
            for mb in range(num_minibatches):
                self.loss_and_grad(env, mb * B, B, k_eps, **hparams)
                self.adam_step(lr)
        self.sync(device_policy, device_value)
        return state, self.metrics(), k_out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.pp3_learner_destroy(self._h)
            self._h = None
            for b in (self._norm, self._metrics, self._eps[1] if self._eps else None):
                if b is not None:
                    b.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
