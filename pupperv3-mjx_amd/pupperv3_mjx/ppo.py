"""Brax PPO's learner step on the device (csrc/pp3_learn.hip; the contract is the comment above
pp3_learner_create in include/pupper_hip.h): compute_ppo_loss's gradients for both networks on a
minibatch of a `PupperV3Env.collect_ppo` batch, Adam, and the reload of the actor and critic
handles from the trained parameters, all on the env's stream without a host round trip.

    learner = PPOLearner(policy_dict, value_dict, normalizer=(mean, std))
    actor, critic = learner.make_policies()
    state, metrics, key = learner.train_iteration(env, state, key, actor, critic, nsteps=20)

Off by default, the rest of Brax's training_step: the running observation normaliser
(`running_statistics=True`, `update_normalizer`), a fresh env permutation per update pass
(`set_env_index`, `loss_and_grad(indexed=True)`; `rng.permutation`) and optax's global-norm clip
(`clip_gradients`); `train_iteration(shuffle=, max_grad_norm=, update_normalizer=)` chains them in
Brax's order.

Across ranks (one process per GPU, `sharding.Comm`): `train_iteration(..., comm=comm)` is Brax's
training_step under pmap.  Every rank collects on its own env shard and differentiates its own
minibatch; `allreduce_gradients(comm)` then replaces the gradients and the metrics by their mean over
the ranks (jax.lax.pmean) before the clip and Adam, and `update_normalizer(env, comm)` adds every
rank's rows to the statistics (running_statistics.update's psums).  Both sums are taken in rank order
from all-gathered contributions (the header's reduction contract), so every rank computes the same
bits and the replicas stay bit-identical for the life of the job, provided that

  * all ranks start from identical parameters and statistics (the same policy_dict, value_dict,
    normalizer) and pass the same hyper-parameters, minibatch counts and nsteps;
  * each rank passes its own key, e.g. `rng.split(key, world)[rank]`, as Brax gives each device its own:
    the collection noise, the entropy noise and the shuffle then differ per rank, as they should.

The mean over ranks is unweighted (Brax's): shards of unequal size weigh their rows unequally.

The two random inputs of an iteration, the entropy noise rng.normal(k_eps, (K, N, 12)) and each update
pass's rng.permutation(k_u, N), are drawn on the host and uploaded by default.  `device_rng=True`
(`train_iteration`, `loss_and_grad`; `draw_entropy_noise`, `shuffle_env_index`) draws both on the
device from the same keys, stream-ordered with no host copy; the scalar key splits stay on the host.
The index is bit-identical to the host path's.  The noise agrees with it to erfinvf rounding: its
uniform is jax's bit for bit on both paths, then the host path rounds scipy's float64 erfinv to f32
where the device evaluates the device library's erfinvf, and neither is bit-pinned to XLA's erf_inv.

The loop around it is `train` (Brax's ppo.train schedule: `eval_schedule`): it resets the training
envs, runs the iterations and evaluates with an `evaluator.Evaluator` before training and after every
epoch, calling `progress_fn` and `policy_params_fn` at each evaluation; `learning_rate` may be a
callable of the iteration index.

    actor, critic, metrics = ppo.train(learner, wrap(env, 1000), wrap(eval_env, 1000), num_timesteps=10_000_000,
                                       episode_length=1000, num_evals=10, key=key, progress_fn=progress)

Initial parameters: `make_learner(key, observation_size, ...)` builds a learner of Brax's
make_ppo_networks shapes and draws lecun_uniform kernels and zero biases on the device
(`PPOLearner.init_params` = pp3_learner_init_params; `init_params` is one net in numpy, the same
bits).  Ranks that pass the same key hold identical parameters without a broadcast.

Checkpoints: `PPOLearner.state_dict` / `load_state_dict` (parameters, Adam's moments, t, the
normaliser), the same pair on PupperV3Env, wrappers.wrap's env and the Evaluator, one atomic .npz of
plain arrays by `save_checkpoint` / `load_checkpoint`, and `train(checkpoint_path=, restore=)`: a run
interrupted at a checkpoint and resumed on fresh objects ends with the bits of the uninterrupted run.

    learner = ppo.make_learner(key, env.observation_size, max_rows=(K + 1) * N)
    ppo.train(learner, env, eval_env, ..., checkpoint_path=lambda steps: f"ck_{steps}.npz")
    ppo.train(learner2, env2, eval_env2, ..., restore="ck_36000000.npz")      # after a crash

Training metrics: `EpisodeStats` rebuilds Brax's EpisodeWrapper record (sum_reward, length) at the done
steps of every collected batch on the device (pp3_episode_stats_*), `train_iteration(episode_stats=)`
feeds it and `train(log_training_metrics=True)` reports episode/sum_reward, episode/length,
episode/truncated and episode/count at every epoch end: a learning curve between evaluations.  Brax
averages a deque of the last 100 finished episodes there; this averages every episode that ended
in the epoch.  Under `comm` the iteration's four sums go through the rank-ordered sum, so every rank
reports the job's numbers; `train(reduce_eval_metrics=True)` does the same for the evaluation
(`Evaluator(comm=)`).  train_iteration collects with `collect_ppo(host_batch=False)`: the batch is
never downloaded, and the iteration's only host wait is the one behind its returned metrics.

Not here (follow-ups): bf16 / mixed precision.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np

from . import _abi, _lib, rng
from .export import DevicePolicy, layers_blob

ROW_CHUNK = 256  # PP3_LEARN_ROW_CHUNK: rows per partial sum of the weight gradient
NORM_RANGES = 1024  # row ranges of the normaliser update's first level: ceil(rows / NORM_RANGES) rows each
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
    .std; None: identity), held on the device with their gradients and Adam moments.
    `running_statistics`: the normaliser is Brax's running_statistics state (mean, std,
    summed_variance on the device, the count a Python int) that `update_normalizer` advances;
    `normalizer` may then also carry .summed_variance and .count, and None starts from Brax's
    initial state (count 0, mean 0, summed_variance 0, std 1)."""

    def __init__(self, policy_dict: Dict[str, Any], value_dict: Dict[str, Any], normalizer=None, device: int = 0,
                 max_rows: int = 21 * 4096, running_statistics: bool = False):
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
        _lib.check(L.pp3_learner_create(
            self.device, pin, len(pout), _vp(pout), _vp(pact), _vp(pblob), len(vout), _vp(vout), _vp(vact), _vp(vblob),
            float(dist["min_std"]), float(dist["var_scale"]), self.max_rows, C.byref(h)), "learn")
        self._h = h
        self._norm = None  # rows: mean, std, summed_variance
        self.running_statistics = bool(running_statistics)
        self._count = 0    # the normaliser's count (running_statistics)
        if normalizer is not None or self.running_statistics:
            sv = np.zeros(pin, np.float32)
            if normalizer is None:
                mean, std = np.zeros(pin, np.float32), np.ones(pin, np.float32)
            elif isinstance(normalizer, (tuple, list)):
                mean, std = normalizer
            else:
                mean, std = normalizer.mean, normalizer.std
                sv = getattr(normalizer, "summed_variance", sv)
                self._count = int(getattr(normalizer, "count", 0))
            rows = [np.asarray(a, np.float32) for a in (mean, std, sv)]
            if any(a.shape != (pin,) for a in rows):
                raise ValueError(f"the normaliser needs mean and std of {pin} entries")
            ms = np.ascontiguousarray(np.stack(rows))
            self._norm = _lib.DeviceBuffer(ms.nbytes, self.device)
            self._norm.upload(ms)
        self._metrics = _lib.DeviceBuffer(16, self.device)
        self._gnorm = _lib.DeviceBuffer(4, self.device)  # the last clip_gradients' norm
        self._eps = None  # (key bytes, shape, DeviceBuffer)
        self._dev_eps = None  # ((key bytes, shape, layout, env), device address): the draw the learner's noise buffer holds
        self._global_rows = (None, {})  # (communicator, {(K, N): rows of all ranks}) behind update_normalizer
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

    def _stream(self, stream=None):
        """`stream`, by default the stream of the env the last call ran on (else the default stream)."""
        if stream is None and self._env is not None:
            stream = self._env._L.pp3_stream(self._env._h)
        return C.c_void_p(stream) if stream else None

    def _check(self, rc: int) -> None:
        _lib.check(rc, "learn")

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
                             entropy_cost: float = 1e-2, normalize_advantage: bool = True,
                             indexed: bool = False) -> None:
        """pp3_ppo_loss_grad on device addresses (arrays of a batch of N envs and K steps, see the header);
        indexed: pp3_ppo_loss_grad_indexed, rows [e0, e0 + B) of the index of set_env_index."""
        p = lambda v: C.c_void_p(v) if v else None
        mean, std = self._norm_ptrs()
        fn = self._L.pp3_ppo_loss_grad_indexed if indexed else self._L.pp3_ppo_loss_grad
        self._check(fn(
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

    def draw_entropy_noise(self, env, key, shape) -> int:
        """jax.random.normal(key, shape = (K, N, 12)) drawn on the device into the learner's noise
        buffer (pp3_learner_draw_noise), on the env's stream; returns the device address, the `eps`
        of loss_and_grad_device.  The next draw overwrites it."""
        K, N, nu = (int(s) for s in shape)
        if nu != _abi.NU:
            raise ValueError(f"the entropy noise has shape (K, N, {_abi.NU})")
        env = _base(env)
        self._env = env
        k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
        out = C.c_void_p()
        self._check(self._L.pp3_learner_draw_noise(self._h, _vp(k), K, N, int(bool(env._partitionable)), C.byref(out),
                                                   self._stream()))
        self._dev_eps = None  # (the buffer no longer holds what a cached draw put there)
        return out.value

    def _dev_eps_for(self, env, eps_key, shape) -> int:
        """_eps_for on the device: one draw per (key, shape), shared by an iteration's minibatches.
        The env is part of the tag: the draw is ordered on that env's stream only, so a call on
        another env draws again on its own stream."""
        k = np.asarray(eps_key, dtype=np.uint32).reshape(2)
        tag = (k.tobytes(), tuple(shape), bool(env._partitionable), env)  # (the env itself: an id could be reused)
        if self._dev_eps is None or self._dev_eps[0] != tag:
            self._dev_eps = (tag, self.draw_entropy_noise(env, k, shape))
        return self._dev_eps[1]

    def shuffle_env_index(self, key, n: int, partitionable: Optional[bool] = None, stream=None) -> None:
        """jax.random.permutation(key, n) drawn on the device into the env index behind
        loss_and_grad(indexed=True) (pp3_learner_shuffle_env_index): rng.permutation's bits with no
        host copy.  partitionable, stream: by default those of the env the last call ran on (else
        jax 0.5's layout, the default stream)."""
        if partitionable is None:
            partitionable = self._env._partitionable if self._env is not None else True
        k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
        self._check(self._L.pp3_learner_shuffle_env_index(self._h, _vp(k), int(n), int(bool(partitionable)),
                                                          self._stream(stream)))

    def rng_buffers(self) -> Dict[str, Tuple[Optional[int], int]]:
        """{"index": (device address or None, entries set), "noise": (device address or None, floats
        allocated)}: the env index and the device-drawn noise (pp3_learner_rng_buffers)."""
        ip, n, zp, cnt = C.c_void_p(), C.c_int32(), C.c_void_p(), C.c_int64()
        self._check(self._L.pp3_learner_rng_buffers(self._h, C.byref(ip), C.byref(n), C.byref(zp), C.byref(cnt)))
        return {"index": (ip.value, n.value), "noise": (zp.value, cnt.value)}

    def env_index(self) -> np.ndarray:
        """The env index as set_env_index or shuffle_env_index left it, downloaded (waits for the stream)."""
        ptr, n = self.rng_buffers()["index"]
        if not n:
            raise ValueError("no env index is set")
        self._wait()
        out = np.empty(n, np.int32)
        _lib.check(self._L.pp3_memcpy_d2h(_vp(out), C.c_void_p(ptr), out.nbytes))
        return out

    def loss_and_grad(self, env, e0: int, B: int, eps_key, indexed: bool = False, device_rng: bool = False,
                      **hparams) -> None:
        """Loss and gradients on envs [e0, e0 + B) of the env's last collect_ppo batch (indexed: on
        the envs index[e0 : e0 + B] of set_env_index), on the env's stream.  hparams: HPARAMS' keys.
        device_rng: the entropy noise of eps_key is drawn on the device (draw_entropy_noise) instead of
        on the host, once per (key, shape) either way.  Results: grads(), metrics()."""
        dev = env.ppo_device_batch()
        ptr, (K, N, D) = dev["observation"]
        if D != self.in_dim:
            raise ValueError(f"the batch's observations have {D} entries, the networks read {self.in_dim}")
        env = _base(env)
        eps = (self._dev_eps_for if device_rng else self._eps_for)(env, eps_key, (K, N, _abi.NU))
        self._env = env
        self.loss_and_grad_device(K, B, N, e0, ptr, dev["raw_action"][0], dev["log_prob"][0], dev["reward"][0],
                                  dev["done"][0], dev["truncation"][0], eps, env._L.pp3_stream(env._h),
                                  **{**HPARAMS, **hparams}, indexed=indexed)

    def set_env_index(self, index, stream=None) -> None:
        """The env index behind loss_and_grad(indexed=True): int32 [num_envs], every entry in
        [0, num_envs) (checked on the host; e.g. rng.permutation).  Copied in stream order."""
        idx = np.ascontiguousarray(np.asarray(index, dtype=np.int32).ravel())
        self._check(self._L.pp3_learner_set_env_index(self._h, _vp(idx), idx.size, self._stream(stream)))

    def allreduce_gradients(self, comm, stream=None) -> None:
        """jax.lax.pmean of the gradients and metrics of the last loss_and_grad over the ranks of
        `comm` (pp3_learner_allreduce_grads: one all-gather, then the rank-ordered sum), between
        loss_and_grad and clip_gradients / adam_step.  Every rank must call it; grads() and metrics()
        then return the rank mean, the same bits on every rank."""
        self._check(self._L.pp3_learner_allreduce_grads(self._h, comm._h, self._metrics.ptr, self._stream(stream)))

    def _rows_of_all_ranks(self, comm, K: int, N: int) -> int:
        """The sum over ranks of K * N, from one host comm.allreduce per (K, N): shard sizes are fixed
        for a communicator's life, so later iterations reuse it."""
        if self._global_rows[0] is not comm:
            self._global_rows = (comm, {})
        cache = self._global_rows[1]
        if (K, N) not in cache:
            cache[(K, N)] = int(round(float(comm.allreduce([float(K * N)], "sum")[0])))
        return cache[(K, N)]

    def update_normalizer(self, env, comm=None, std_min: float = 1e-6, std_max: float = 1e6) -> None:
        """Brax's running_statistics.update with the observations the actor saw in the env's last
        collect_ppo batch ([K][N][36H]; the bootstrap row is not read), on the env's stream.  comm:
        with the rows of every rank's batch (pp3_learner_normalizer_update_ranks; every rank must
        call it), the count advancing by all ranks' rows."""
        if not self.running_statistics:
            raise ValueError("update_normalizer needs PPOLearner(running_statistics=True)")
        ptr, (K, N, D) = env.ppo_device_batch()["observation"]
        if D != self.in_dim:
            raise ValueError(f"the batch's observations have {D} entries, the networks read {self.in_dim}")
        self._env = _base(env)
        base = self._norm.ptr.value
        state = (C.c_void_p(base), C.c_void_p(base + 8 * self.in_dim), C.c_void_p(base + 4 * self.in_dim))
        if comm is None:
            count = self._count + K * N
            self._check(self._L.pp3_learner_normalizer_update(
                self._h, C.c_void_p(ptr), K * N, float(np.float32(count)), float(std_min), float(std_max), *state,
                self._stream()))
        else:
            count = self._count + self._rows_of_all_ranks(comm, K, N)
            self._check(self._L.pp3_learner_normalizer_update_ranks(
                self._h, comm._h, C.c_void_p(ptr), K * N, float(np.float32(count)), float(std_min), float(std_max),
                *state, self._stream()))
        self._count = count

    def normalizer_state(self) -> Dict[str, Any]:
        """dict(mean, std, summed_variance, count) downloaded (export, checkpoints); waits for the stream."""
        if self._norm is None:
            raise ValueError("this learner has no normaliser")
        self._wait()
        ms = np.empty((3, self.in_dim), np.float32)
        self._norm.download(ms)
        return dict(mean=ms[0], std=ms[1], summed_variance=ms[2], count=self._count)

    def clip_gradients(self, max_norm: float, stream=None) -> None:
        """optax.clip_by_global_norm on the gradients of the last loss_and_grad (pp3_grad_clip),
        before adam_step; the norm: grad_norm()."""
        self._check(self._L.pp3_grad_clip(self._h, float(max_norm), self._gnorm.ptr, self._stream(stream)))

    def grad_norm(self) -> float:
        """The global gradient norm the last clip_gradients measured (before clipping; waits for it)."""
        self._wait()
        out = np.empty(1, np.float32)
        self._gnorm.download(out)
        return float(out[0])

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

    # ---- initialisation and checkpoints -------------------------------------------------------
    def _drop_noise(self) -> None:
        """Forgets the cached entropy-noise draws (the next loss_and_grad draws again)."""
        self._dev_eps = None
        if self._eps is not None:
            self._eps[1].free()
            self._eps = None

    def init_params(self, key, partitionable: Optional[bool] = None) -> None:
        """Brax's initial networks drawn on the device from `key` (pp3_learner_init_params: lecun_uniform
        kernels, zero biases; the key schedule and the numpy restatement: `ppo.init_params`), on the
        stream of the env the last call ran on (else the default stream).  The gradients and both Adam
        moments become zero, t = 0, a running_statistics normaliser returns to Brax's initial state
        (count 0, mean 0, summed_variance 0, std 1) and the cached noise draw is dropped.  Handles made
        earlier keep their weights until `sync`.  partitionable: by default that env's (else jax 0.5's
        layout).  Ranks that pass the same key hold the same bits; no broadcast is needed."""
        if partitionable is None:
            partitionable = self._env._partitionable if self._env is not None else True
        k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
        self._check(self._L.pp3_learner_init_params(self._h, _vp(k), int(bool(partitionable)), self._stream()))
        self.t = 0
        if self.running_statistics:
            self._wait()
            self._norm.upload(np.stack([np.zeros(self.in_dim, np.float32), np.ones(self.in_dim, np.float32),
                                        np.zeros(self.in_dim, np.float32)]))
            self._count = 0
        self._drop_noise()

    def _describe(self) -> Dict[str, np.ndarray]:
        """What a state_dict's blobs depend on (compared at load)."""
        (pin, pout, pact), (_, vout, vact) = self._shapes
        return {"in_dim": np.asarray(pin, np.int64),
                "policy_widths": np.asarray(pout, np.int32), "policy_activations": np.asarray(pact, np.int32),
                "value_widths": np.asarray(vout, np.int32), "value_activations": np.asarray(vact, np.int32),
                "min_std": np.asarray(self.distribution["min_std"], np.float32),
                "var_scale": np.asarray(self.distribution["var_scale"], np.float32),
                "running_statistics": np.asarray(self.running_statistics, np.bool_),
                "has_normalizer": np.asarray(self._norm is not None, np.bool_)}

    _BLOBS = tuple((f"{name}_{what}", net, which) for net, name in ((0, "policy"), (1, "value"))
                   for which, what in ((0, "params"), (2, "m"), (3, "v")))

    def state_dict(self) -> Dict[str, np.ndarray]:
        """Everything an iteration reads that an earlier one wrote, as plain arrays (waits for the
        stream): per net the parameter blob and Adam's m and v (flat f32, the layout of `buffer`), t,
        and with a normaliser its rows mean | std | summed_variance [3][in_dim] and the count; beside
        them the shapes and flags `load_state_dict` compares.  Not state, because train_iteration
        rewrites each before it reads it: the gradients (every loss_and_grad stores all of both blobs
        before the clip or Adam reads them), the workspaces, the metrics, the env index (set by each
        shuffled pass before the indexed loss reads it; unshuffled passes never read it) and the noise
        buffer (drawn at an iteration's first loss_and_grad, the cache being dropped at load)."""
        d = self._describe()
        for name, net, which in self._BLOBS:
            d[name] = self._download(net, which)
        d["t"] = np.asarray(self.t, np.int64)
        if self._norm is not None:
            ns = self.normalizer_state()
            d["normalizer"] = np.stack([ns["mean"], ns["std"], ns["summed_variance"]])
            d["count"] = np.asarray(ns["count"], np.int64)
        return d

    def load_state_dict(self, d: Dict[str, np.ndarray]) -> None:
        """Puts a `state_dict` back: ValueError, with nothing touched, when a shape, an activation,
        min_std, var_scale, running_statistics or the presence of a normaliser differs from this
        learner's or an array is missing or misshapen; else the blobs are uploaded behind the stream's
        queued work, t and the count set, and the cached noise draw dropped.  Handles made earlier
        keep their weights until `sync` (make_policies after a load returns loaded ones)."""
        for k, v in self._describe().items():
            if k not in d or not np.array_equal(np.asarray(d[k]), v):
                raise ValueError(f"the state_dict is of another learner: {k} is {d.get(k)}, this learner's is {v}")
        want = {name: (self.buffer(net, which)[1],) for name, net, which in self._BLOBS}
        if self._norm is not None:
            want["normalizer"] = (3, self.in_dim)
        arrays = {}
        for name, shape in want.items():
            a = np.asarray(d[name]) if name in d else None
            if a is None or a.dtype != np.float32 or a.shape != shape:
                raise ValueError(f"the state_dict's {name} must be float32 {shape}")
            arrays[name] = np.ascontiguousarray(a)
        for name in ("t",) + (("count",) if self._norm is not None else ()):
            if name not in d or int(d[name]) < 0:
                raise ValueError(f"the state_dict lacks {name}")
        self._wait()
        for name, net, which in self._BLOBS:
            a = arrays[name]
            _lib.check(self._L.pp3_memcpy_h2d(C.c_void_p(self.buffer(net, which)[0]), _vp(a), a.nbytes))
        if self._norm is not None:
            self._norm.upload(arrays["normalizer"])
            self._count = int(d["count"])
        self.t = int(d["t"])
        self._drop_noise()

    def make_policies(self) -> Tuple[DevicePolicy, DevicePolicy]:
        """(actor, critic) handles of the networks' shapes, loaded with the current parameters."""
        actor, critic = DevicePolicy(self._dicts[0], self.device), DevicePolicy(self._dicts[1], self.device)
        self.sync(actor, critic)
        return actor, critic

    def deterministic_policy(self) -> DevicePolicy:
        """A deployment handle of the current parameters (12 outputs: tanh of the head's mean, the
        normaliser folded into layer 0 on the host in f32), for a deterministic evaluation.  It is a
        snapshot built from downloads (waits for the stream); the caller closes it."""
        layers = self.params()["policy"]
        if self._norm is not None:
            ns = self.normalizer_state()
            inv = np.float32(1.0) / ns["std"].astype(np.float32)
            k0, b0 = layers[0]
            layers[0] = ((k0 * inv[:, None]).astype(np.float32),
                         (b0 - (ns["mean"].astype(np.float32) * inv) @ k0).astype(np.float32))
        kl, bl = layers[-1]
        layers[-1] = (np.ascontiguousarray(kl[:, :_abi.NU]), np.ascontiguousarray(bl[:_abi.NU]))
        src = self._dicts[0]
        out = {k: v for k, v in src.items() if k not in ("layers", "distribution")}
        out["layers"] = []
        for i, (layer, (k, b)) in enumerate(zip(src["layers"], layers)):
            last = i == len(layers) - 1
            out["layers"].append(dict(layer, weights=[k, b], shape=[None, int(b.shape[0])],
                                      activation="tanh" if last else layer["activation"]))
        return DevicePolicy(out, self.device)

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
                        num_minibatches: int = 1, num_updates_per_batch: int = 1, lr: float = 3e-4,
                        shuffle: bool = False, max_grad_norm: Optional[float] = None, update_normalizer: bool = False,
                        comm=None, device_rng: bool = False, episode_stats: Optional["EpisodeStats"] = None, **hparams):
        """One PPO iteration in Brax's training_step order: collect_ppo with the handles (the old
        parameters and statistics), update_normalizer: the running statistics, then
        num_updates_per_batch passes over num_minibatches minibatches (loss, gradient, max_grad_norm:
        the clip, Adam each) with the new statistics, then the reload.  Minibatches are contiguous
        env ranges, or with shuffle ranges [mb B, (mb + 1) B) of a fresh rng.permutation per pass.
        key -> (collect key, entropy-noise key) by rng.split; with shuffle k_perm = split(entropy-
        noise key)[1] and per pass k_perm, k_u = split(k_perm), the pass's index from k_u.  Returns
        (state, metrics of the last minibatch, the collect's key chain end).
        device_rng: the same keys feed the same draws, on the device: the entropy noise from the
        entropy-noise key (draw_entropy_noise, once) and each pass's index from its k_u
        (shuffle_env_index); only the scalar key splits stay on the host.  The index is the host
        path's bit for bit, the noise agrees with it to erfinvf rounding (module docstring).
        comm (a sharding.Comm; every rank makes the same call on its own env shard with its own key,
        see the module docstring): the statistics take every rank's rows, allreduce_gradients runs
        between the loss and the clip, and the metrics are the mean over ranks.
        episode_stats (an EpisodeStats): `begin` is queued before the collect and `add` after it (under
        comm with the rank sum, so every rank accumulates the job's numbers); its 16 bytes are
        downloaded behind the wait the returned metrics make.  The collect is
        collect_ppo(host_batch=False): no batch download and no other host wait in the iteration."""
        base = _base(env)
        n = base.num_envs
        if n % num_minibatches:
            raise ValueError(f"{n} envs do not divide into {num_minibatches} minibatches")
        B = n // num_minibatches
        k_collect, k_eps = rng.split(np.asarray(key, dtype=np.uint32).reshape(2), 2, base._partitionable)
        gae = {k: hparams[k] for k in ("discount", "gae_lambda", "reward_scaling") if k in hparams}
        if episode_stats is not None:
            if not base.holds(state):  # an edited state: on the device first, as the collect would put it
                if env is not base:
                    env._prepare(state)
                base._write_state(state)
            episode_stats.begin(env)
        state, _, k_out = env.collect_ppo(state, device_policy, device_value, nsteps, k_collect, host_batch=False, **gae)
        if episode_stats is not None:
            episode_stats.add(env, comm)
        if update_normalizer:
            self.update_normalizer(env, comm)
        k_perm = rng.split(k_eps, 2, base._partitionable)[1] if shuffle else None
        for _ in range(num_updates_per_batch):
            if shuffle:
                k_perm, k_u = rng.split(k_perm, 2, base._partitionable)
                self._env = base
                if device_rng:
                    self.shuffle_env_index(k_u, n, base._partitionable)
                else:
                    self.set_env_index(rng.permutation(k_u, n, base._partitionable))
            for mb in range(num_minibatches):
                self.loss_and_grad(env, mb * B, B, k_eps, indexed=bool(shuffle), device_rng=device_rng, **hparams)
                if comm is not None:
                    self.allreduce_gradients(comm)
                if max_grad_norm is not None:
                    self.clip_gradients(max_grad_norm)
                self.adam_step(lr)
        self.sync(device_policy, device_value)
        metrics = self.metrics()
        if episode_stats is not None:
            episode_stats.fetch()  # (metrics() has waited for the stream)
        return state, metrics, k_out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.pp3_learner_destroy(self._h)
            self._h = None
            self._dev_eps = None
            for b in (self._norm, self._metrics, self._gnorm, self._eps[1] if self._eps else None):
                if b is not None:
                    b.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EpisodeStats:
    """Training episode statistics: Brax's EpisodeWrapper episode_metrics (sum_reward, length) and
    the truncation flag at the done steps of collected batches (the contract: "Training episode
    statistics" in include/pupper_hip.h).  Owns the device buffers carry [3][N], part [4][N] and out4
    and the host accumulators.

        stats = EpisodeStats()
        stats.begin(env); env.collect_ppo(...); stats.add(env)      # per batch, all queued, no wait
        count, sums = stats.read()                                    # waits, then downloads 16 bytes

    `env`: a wrappers.wrap'ped env (ValueError otherwise), always the same one.  `begin` seeds the
    carry from the env's episode record and done flags, so it must be queued after the state the
    collect starts from is on the device and before the collect; `add` chains over the batch's
    reward / done / truncation rows (`env.ppo_device_batch()`).  With `comm` (every rank calls) the
    batch's four sums are summed over the ranks in rank order first.  Each batch's f32 (episodes,
    sum of returns, sum of lengths, truncated episodes) is added to the host accumulators in batch
    order: the count a Python int, the sums Python floats.  `read()` -> (count, {"sum_reward",
    "length", "truncated"}); `reset()` empties the accumulators.  Nothing here is training state:
    the carry is re-seeded from the env at every `begin`."""

    def __init__(self):
        self._L = _lib.load()
        self._bufs = None  # (n, device, carry, part, out4 | its rank sum)
        self._env = None
        self._pending = False  # an add() whose out4 has not been downloaded yet
        self._src = 0          # byte offset of the numbers to download: out4, or its rank sum behind it
        self.last = None       # the last downloaded batch's four f32
        self.reset()

    def reset(self) -> None:
        self.count, self.sum_reward, self.length, self.truncated = 0, 0.0, 0.0, 0.0

    def _check(self, rc: int) -> None:
        _lib.check(rc, "ppo")

    def _buffers(self, env):
        base = getattr(env, "env", None)
        if base is None or not hasattr(env, "action_repeat"):
            raise ValueError("EpisodeStats needs a wrapped env (wrappers.wrap: EpisodeWrapper + AutoResetWrapper)")
        if self._bufs is None or self._bufs[:2] != (base.num_envs, base.device):
            self.close()
            n, dev = base.num_envs, base.device
            self._bufs = (n, dev, _lib.DeviceBuffer(4 * 3 * n, dev), _lib.DeviceBuffer(4 * 4 * n, dev),
                          _lib.DeviceBuffer(4 * 8, dev))
        self._env = base
        return base, self._bufs

    def begin(self, env) -> None:
        """Seeds the carry from the env's record (pp3_episode_stats_begin on the env's stream)."""
        if self._pending:
            self.read()
        base, (n, dev, carry, _, _) = self._buffers(env)
        ep, stride = base.device_field(_abi.F_EPISODE)
        done, _ = base.device_field(_abi.F_DONE)
        self._check(self._L.pp3_episode_stats_begin(dev, n, C.c_void_p(ep), stride, C.c_void_p(done), carry.ptr,
                                                    C.c_void_p(base._L.pp3_stream(base._h))))

    def add(self, env, comm=None) -> None:
        """The last collect_ppo batch's rows (pp3_episode_stats_rows on the env's stream; with comm,
        then the rank sum of out4).  Nothing waits; `fetch` / `read` pick the result up."""
        if self._pending:
            raise ValueError("EpisodeStats.add: the previous batch was not read (begin() or read() first)")
        base, (n, dev, carry, part, out) = self._buffers(env)
        b = env.ppo_device_batch()
        (rew, (K, nb)), (done, _), (trunc, _) = b["reward"], b["done"], b["truncation"]
        if nb != n:
            raise ValueError(f"the batch has {nb} envs, the statistics {n}")
        stream = base._L.pp3_stream(base._h)
        self._check(self._L.pp3_episode_stats_rows(dev, K, n, n, C.c_void_p(rew), C.c_void_p(done), C.c_void_p(trunc),
                                                   int(env.action_repeat), carry.ptr, part.ptr, out.ptr,
                                                   C.c_void_p(stream)))
        self._src = 0
        if comm is not None:
            comm.sum_ranks_device(out.ptr.value, out.ptr.value + 16, 4, stream)
            self._src = 16
        self._pending = True

    def fetch(self) -> None:
        """Downloads the pending batch's four numbers and adds them to the accumulators; the caller
        has already waited for the env's stream (train_iteration: behind metrics()' wait)."""
        if not self._pending:
            return
        out = np.empty(4, np.float32)
        _lib.check(self._L.pp3_memcpy_d2h(_vp(out), C.c_void_p(self._bufs[4].ptr.value + self._src), out.nbytes))
        self._pending = False
        self.last = out
        self.count += int(out[0])
        self.sum_reward += float(out[1])
        self.length += float(out[2])
        self.truncated += float(out[3])

    def read(self) -> Tuple[int, Dict[str, float]]:
        """(episodes finished, {"sum_reward", "length", "truncated"}: their sums) since the last reset()."""
        if self._pending:
            self._env.synchronize()
            self.fetch()
        return self.count, {"sum_reward": self.sum_reward, "length": self.length, "truncated": self.truncated}

    def local_out4(self) -> np.ndarray:
        """This rank's own four numbers of the last add() (before the rank sum); waits for the stream."""
        self._env.synchronize()
        out = np.empty(4, np.float32)
        self._bufs[4].download(out)
        return out

    def carry(self) -> np.ndarray:
        """The carry [3][N] (ret, len, pd) downloaded; waits for the stream."""
        self._env.synchronize()
        out = np.empty((3, self._bufs[0]), np.float32)
        self._bufs[2].download(out)
        return out

    def metrics(self) -> Dict[str, float]:
        """The episode/* keys of a report: the means over the finished episodes, the truncated
        fraction and the count; with no episode, the count only."""
        count, sums = self.read()
        m: Dict[str, float] = {"episode/count": count}
        if count:
            m.update({"episode/sum_reward": sums["sum_reward"] / count, "episode/length": sums["length"] / count,
                      "episode/truncated": sums["truncated"] / count})
        return m

    def close(self) -> None:
        if self._bufs is not None:
            for b in self._bufs[2:]:
                b.free()
            self._bufs = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def init_params(key, in_dim: int, hidden, out: int, partitionable: bool = True) -> List[Tuple[np.ndarray, np.ndarray]]:
    """One network's initial [(kernel [in][out], bias [out]), ...] from its net key, in numpy: the
    contract above pp3_learner_init_params in include/pupper_hip.h, which the device entry equals bit
    for bit.  Layers in_dim -> hidden.. -> out; for layer l in order `key, k_l = rng.split(key)`, the
    kernel rng.uniform(k_l, (fan_in, width), -1, 1) * s with s = sqrt(3 * (1 / fan_in)) in float32
    (jax's lecun_uniform: variance 1 / fan_in), the bias zero.  A learner's two net keys are
    `k_policy, k_value = rng.split(key)` of the key given to PPOLearner.init_params / make_learner.
    The schedule is this library's own: flax folds module paths into the key, which cannot be
    pinned here, so the distribution is Brax's and the stream behind it is not."""
    k_net = np.asarray(key, dtype=np.uint32).reshape(2)
    layers, fan_in = [], int(in_dim)
    for width in tuple(int(m) for m in hidden) + (int(out),):
        k_net, k_l = rng.split(k_net, 2, partitionable)
        s = np.sqrt(np.float32(3.0) * (np.float32(1.0) / np.float32(fan_in)))
        u = rng.uniform(k_l, (fan_in, width), -1.0, 1.0, partitionable)
        layers.append(((u * np.float32(s)).astype(np.float32), np.zeros(width, np.float32)))
        fan_in = width
    return layers


def make_learner(key, observation_size: int, policy_hidden_layer_sizes=(256, 128, 128),
                 value_hidden_layer_sizes=(256, 128, 128), activation: str = "elu", min_std: float = 0.001,
                 var_scale: float = 1.0, running_statistics: bool = True, max_rows: int = 21 * 4096, device: int = 0,
                 **export_metadata) -> PPOLearner:
    """A PPOLearner of Brax's make_ppo_networks shapes (the policy's last layer the 24-column
    normal_tanh head, the value net's one column, both un-folded) with Brax's initial parameters
    drawn on the device from `key` (PPOLearner.init_params, in jax 0.5's counter layout; for an env
    of rng_partitionable=False call `init_params(key, False)` again).  export_metadata: none, or all of
    export.METADATA_KEYS (convert_params' arguments: action scale, kp, kd, poses, limits, use_imu,
    observation_history, pitch / roll maxima), kept beside the layers so that `deterministic_policy()`
    and a JSON export of it carry them."""
    from .export import zero_network_dicts
    pol, val = zero_network_dicts(observation_size, policy_hidden_layer_sizes, value_hidden_layer_sizes, activation,
                                  min_std, var_scale, **export_metadata)
    learner = PPOLearner(pol, val, device=device, max_rows=max_rows, running_statistics=running_statistics)
    learner.init_params(key)
    return learner


# ---- checkpoints ------------------------------------------------------------------------------
CHECKPOINT_PARTS = ("learner", "env", "evaluator", "loop")


def _part(obj) -> Dict[str, np.ndarray]:
    """A checkpoint part: an object's state_dict(), or a mapping of arrays as it is."""
    d = obj.state_dict() if hasattr(obj, "state_dict") else obj
    out = {}
    for k, v in d.items():
        a = np.asarray(v)
        if a.dtype == object or "/" in k:
            raise ValueError(f"a checkpoint holds plain arrays under names without '/': {k!r}")
        out[k] = a
    return out


def save_checkpoint(path, learner, env, state=None, evaluator=None, loop: Optional[Dict[str, Any]] = None) -> None:
    """One .npz of plain arrays (scalars as 0-d arrays; no pickled object) under "<part>/<name>": the
    state_dict() of the learner, of the training env (a wrappers.wrap'ped env or a PupperV3Env) and
    of the evaluator, and `loop`, what `train` needs to continue (its key chain, the iteration and
    epoch indices, the walltime, the schedule).  `state`: the env State to save; the device usually
    holds it, an edited one is written back first as a step would.  Each of learner / env / evaluator
    may also be a mapping of arrays.  The file is written under a temporary name in the same
    directory and renamed over `path` (os.replace), so a killed job leaves the last complete
    checkpoint, never a partial one."""
    if state is not None and hasattr(env, "state_dict"):
        base = _base(env)
        if not base.holds(state):
            if env is not base:
                env._prepare(state)
            base._write_state(state)
    arrays = {}
    for name, obj in zip(CHECKPOINT_PARTS, (learner, env, evaluator, loop)):
        if obj is not None:
            arrays.update({f"{name}/{k}": v for k, v in _part(obj).items()})
    path = os.fspath(path)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **arrays)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def load_checkpoint(path) -> Dict[str, Dict[str, np.ndarray]]:
    """{"learner" | "env" | "evaluator" | "loop": {name: array}} of a save_checkpoint file (the parts
    it was given), read with allow_pickle=False; each part is what that object's load_state_dict
    takes."""
    out: Dict[str, Dict[str, np.ndarray]] = {}
    with np.load(os.fspath(path), allow_pickle=False) as z:
        for full in z.files:
            part, _, name = full.partition("/")
            if part not in CHECKPOINT_PARTS or not name:
                raise ValueError(f"{path}: not a checkpoint of this library (entry {full!r})")
            out.setdefault(part, {})[name] = z[full]
    return out


def _loop_schedule(sched: Dict[str, Any], unroll_length: int, num_minibatches: int,
                   num_updates_per_batch: int) -> Dict[str, np.ndarray]:
    d = {f"schedule_{k}": np.asarray(v, dtype=np.int64) for k, v in sched.items()}
    d.update(unroll_length=np.asarray(unroll_length, np.int64), num_minibatches=np.asarray(num_minibatches, np.int64),
             num_updates_per_batch=np.asarray(num_updates_per_batch, np.int64))
    return d


def eval_schedule(num_timesteps: int, num_envs: int, unroll_length: int, action_repeat: int = 1,
                  num_evals: int = 1) -> Dict[str, Any]:
    """Brax ppo.train's schedule ([ext] brax 0.12.1 training/agents/ppo/train.py, from memory), with one
    training_step per iteration: an iteration is num_envs * unroll_length * action_repeat env steps;
    num_evals_after_init = max(num_evals - 1, 1) epochs of iterations_per_epoch = ceil(num_timesteps /
    (num_evals_after_init * steps_per_iteration)) iterations each; one evaluation before training when
    num_evals > 1 and one after every epoch.  eval_steps: the env-step count reported at each evaluation."""
    if min(num_timesteps, num_envs, unroll_length, action_repeat, num_evals) < 1:
        raise ValueError("num_timesteps, num_envs, unroll_length, action_repeat and num_evals must be >= 1")
    spi = int(num_envs) * int(unroll_length) * int(action_repeat)
    after = max(int(num_evals) - 1, 1)
    ipe = int(math.ceil(int(num_timesteps) / (after * spi)))
    first = int(num_evals) > 1
    return dict(steps_per_iteration=spi, num_evals_after_init=after, iterations_per_epoch=ipe,
                eval_before_training=first, total_iterations=after * ipe,
                eval_steps=([0] if first else []) + [(e + 1) * ipe * spi for e in range(after)])


def train(learner: PPOLearner, env, eval_env=None, *, num_timesteps: int, episode_length: int, action_repeat: int = 1,
          unroll_length: int = 20, num_minibatches: int = 1, num_updates_per_batch: int = 1,
          learning_rate: Union[float, Callable[[int], float]] = 3e-4, num_evals: int = 1,
          deterministic_eval: bool = False, key, progress_fn: Optional[Callable[[int, Dict[str, Any]], None]] = None,
          policy_params_fn: Optional[Callable[..., None]] = None, shuffle: bool = True,
          max_grad_norm: Optional[float] = None, normalize_observations: bool = False, device_rng: bool = True,
          comm=None, checkpoint_path=None, restore=None, log_training_metrics: bool = False,
          reduce_eval_metrics: bool = False, **hparams):
    """Brax's ppo.train loop around `learner.train_iteration` (the schedule: eval_schedule).  `env`
    and `eval_env` are `wrappers.wrap`ped envs of this `episode_length` / `action_repeat`; `eval_env`
    may also be a constructed `evaluator.Evaluator` (e.g. one on the reward path), or None to train
    without evaluations.  Returns (actor, critic, metrics of the last evaluation or iteration).

    Keys: k_train, k_env, k_eval = split(key, 3); the training envs reset with split(k_env, N); the
    evaluator owns k_eval; iteration i takes `k_train, k_it = split(k_train)` and runs
    train_iteration(key=k_it, lr=learning_rate(i) if callable).  At each evaluation
    progress_fn(num_steps, metrics) and policy_params_fn(num_steps, learner.params(), normaliser
    state or None) are called; metrics = the evaluator's dict with the last iteration's losses as
    training/<name>, training/sps and training/walltime.  deterministic_eval: the evaluation runs
    `learner.deterministic_policy()`, rebuilt from the parameters at every evaluation; otherwise it
    samples from the actor.  normalize_observations: train_iteration(update_normalizer=True), which
    needs PPOLearner(running_statistics=True).  comm: every rank trains on its own shard with its own
    key and evaluates its own eval env; the evaluation metrics are this rank's unless
    reduce_eval_metrics, which hands comm to the Evaluator that train builds: its mean / std keys then
    cover all ranks' eval envs, every env weighing the same (evaluator's docstring).

    log_training_metrics: at every epoch end the metrics gain episode/sum_reward and episode/length
    (means over the episodes that ended in the epoch's rollouts), episode/truncated (their fraction
    the episode length ended) and episode/count; with no finished episode, episode/count only.  The
    accumulators (an EpisodeStats, summed over ranks under comm) then reset.  Brax reports the mean of
    a deque of the last 100 episodes instead.  With eval_env=None, progress_fn(num_steps, metrics) is
    then called at every epoch end with the training metrics (Brax's run_evals=False).

    checkpoint_path (a path, or a callable of num_steps returning one): after every evaluation --
    without an evaluator at the same epoch boundaries -- and after progress_fn and policy_params_fn,
    `save_checkpoint` writes the learner, the training env with the state the next epoch starts from,
    the evaluator's key and the loop (k_train, the iteration and epoch indices, the walltime, the
    schedule).  restore (such a file's path, or `load_checkpoint`'s dict): instead of resetting the
    envs and evaluating once, the learner, the env and the evaluator are loaded and training continues
    at the saved epoch with the saved k_train and iteration index (a callable learning_rate sees the
    continuing index); a run interrupted at a checkpoint and resumed, in a fresh process on fresh
    objects built with the same arguments, ends with the bits of the uninterrupted run.  ValueError
    before anything is loaded when the saved schedule (eval_schedule's dict, unroll_length,
    num_minibatches, num_updates_per_batch) is not the one these arguments give; `key` is not read
    for the continuation.  Under comm every rank saves and restores its own file (its env shard and
    keys differ, the learner part is identical): the caller puts the rank in the path; no
    collective is added.  Domain randomisation and terrain are configuration the caller sets as at
    first."""
    from .evaluator import Evaluator
    base = _base(env)
    n, part = base.num_envs, base._partitionable
    for e in (env,) + (() if eval_env is None or isinstance(eval_env, Evaluator) else (eval_env,)):
        if (getattr(e, "episode_length", None), getattr(e, "action_repeat", None)) != (int(episode_length),
                                                                                      int(action_repeat)):
            raise ValueError("train needs wrappers.wrap'ped envs of the given episode_length and action_repeat")
    sched = eval_schedule(num_timesteps, n, unroll_length, action_repeat, num_evals)
    loop_sched = _loop_schedule(sched, unroll_length, num_minibatches, num_updates_per_batch)
    ck = None
    if restore is not None:
        ck = restore if isinstance(restore, dict) else load_checkpoint(restore)
        saved = ck.get("loop")
        if saved is None or any(k not in saved for k in ("k_train", "iteration", "epoch", "walltime")):
            raise ValueError("restore: the checkpoint has no training loop part (save_checkpoint(loop=...))")
        for k, v in loop_sched.items():
            if k not in saved or not np.array_equal(np.asarray(saved[k]), v):
                raise ValueError(f"restore: the checkpoint was written under another schedule: {k} is "
                                 f"{saved.get(k)}, these arguments give {v}")
        if "learner" not in ck or "env" not in ck or (eval_env is not None and "evaluator" not in ck):
            raise ValueError("restore: the checkpoint lacks the learner, the env or the evaluator")
    k_train, k_env, k_eval = rng.split(np.asarray(key, dtype=np.uint32).reshape(2), 3, part)
    if ck is None:
        state = env.reset(rng.split(k_env, n, part))
        actor, critic = learner.make_policies()
    else:
        learner.load_state_dict(ck["learner"])
        actor, critic = learner.make_policies()
        state = env.load_state_dict(ck["env"])  # (it ends with a device-wide wait: the handles are loaded)
    if eval_env is None:
        evaluator = None
    elif isinstance(eval_env, Evaluator):
        evaluator = eval_env
    else:
        evaluator = Evaluator(eval_env, actor, episode_length, action_repeat, key=k_eval,
                              deterministic=deterministic_eval, comm=comm if reduce_eval_metrics else None)
    stats = EpisodeStats() if log_training_metrics else None
    metrics: Dict[str, Any] = {}
    walltime = 0.0
    it, epoch0 = 0, 0
    if ck is not None:
        if evaluator is not None:
            evaluator.load_state_dict(ck["evaluator"])
        k_train = np.array(np.asarray(ck["loop"]["k_train"], dtype=np.uint32).reshape(2))
        it, epoch0, walltime = int(ck["loop"]["iteration"]), int(ck["loop"]["epoch"]), float(ck["loop"]["walltime"])

    def checkpoint(num_steps: int, next_epoch: int) -> None:
        path = checkpoint_path(num_steps) if callable(checkpoint_path) else checkpoint_path
        loop = dict(loop_sched, k_train=np.asarray(k_train, dtype=np.uint32), iteration=np.asarray(it, np.int64),
                    epoch=np.asarray(next_epoch, np.int64), walltime=np.asarray(walltime, np.float64))
        save_checkpoint(path, learner, env, state, evaluator, loop)

    def evaluate(num_steps: int, training_metrics: Dict[str, Any]) -> Dict[str, Any]:
        pol = learner.deterministic_policy() if evaluator.deterministic else actor
        try:
            m = evaluator.run_evaluation(training_metrics, policy=pol)
        finally:
            if pol is not actor:
                pol.close()
        if progress_fn is not None:
            progress_fn(num_steps, m)
        if policy_params_fn is not None:
            policy_params_fn(num_steps, learner.params(), learner.normalizer_state() if learner._norm is not None else None)
        return m

    if ck is None and evaluator is not None and sched["eval_before_training"]:
        metrics = evaluate(0, {})
        if checkpoint_path is not None:
            checkpoint(0, 0)
    for epoch in range(epoch0, sched["num_evals_after_init"]):
        t0 = time.time()
        for _ in range(sched["iterations_per_epoch"]):
            k_train, k_it = rng.split(k_train, 2, part)
            lr = learning_rate(it) if callable(learning_rate) else learning_rate
            state, losses, _ = learner.train_iteration(
                env, state, k_it, actor, critic, unroll_length, num_minibatches=num_minibatches,
                num_updates_per_batch=num_updates_per_batch, lr=float(lr), shuffle=shuffle, max_grad_norm=max_grad_norm,
                update_normalizer=normalize_observations, comm=comm, device_rng=device_rng, episode_stats=stats,
                **hparams)
            it += 1
        dt = time.time() - t0  # (train_iteration's metrics download has waited for the epoch's work)
        walltime += dt
        metrics = {f"training/{k}": v for k, v in losses.items()}
        metrics["training/sps"] = sched["iterations_per_epoch"] * sched["steps_per_iteration"] / dt
        metrics["training/walltime"] = walltime
        if stats is not None:
            metrics.update(stats.metrics())
            stats.reset()
        if evaluator is not None:
            metrics = evaluate(it * sched["steps_per_iteration"], metrics)
        elif stats is not None and progress_fn is not None:
            progress_fn(it * sched["steps_per_iteration"], metrics)
        if checkpoint_path is not None:
            checkpoint(it * sched["steps_per_iteration"], epoch + 1)
    if evaluator is not None and evaluator is not eval_env:
        evaluator.close()
    if stats is not None:
        stats.close()
    return actor, critic, metrics
