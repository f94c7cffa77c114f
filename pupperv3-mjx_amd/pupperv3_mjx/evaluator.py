"""Brax's Evaluator on the device ([ext] brax 0.12.1 training/acting.py Evaluator over
envs/wrappers/training.py EvalWrapper, restated from memory; the recurrence and the reduction order in
include/pupper_hip.h, "PPO evaluation", are the contract).

    evaluator = Evaluator(wrap(eval_env, 1000), policy, episode_length=1000, key=key)
    metrics = evaluator.run_evaluation(training_metrics)   # {"eval/episode_reward": ..., ...}

One evaluation resets the eval envs, unrolls `episode_length // action_repeat` wrapper steps with the
policy in the loop and reports the mean and the population std over the envs of each env's first
episode: the sums of the reward and of the 19 per-step metrics up to and including its first done
step, and its length.  Everything is queued on the env's stream; the host waits once, for the 42
reduced numbers.

The step kernel keeps no metrics trajectory, so there are two paths, which agree bit for bit on
what both compute:

  * `metrics=True` (per step): one-step `pp3_rollout_policy[_sample]` launches, each followed by
    `pp3_eval_accumulate` on the env's reward / done / metrics / episode buffers: all 20 columns.
  * `metrics=False` (fused): launches of up to `chunk` steps with reward and done trajectories only,
    each followed by `pp3_eval_accumulate_rows`: `eval/episode_reward` and the length keys only.

`deterministic=True` needs a deployment policy (12 outputs, tanh of the mean: `export.convert_params`,
`PPOLearner.deterministic_policy`); `deterministic=False` samples from a training policy
(`export.convert_training_params`, the learner's actor) with `generate_unroll`'s key chain.

Across ranks (`comm`, a sharding.Comm; every rank evaluates its own eval env shard and makes the same
calls): the mean / std keys are over the eval envs of all ranks.  pp3_eval_reduce is cut where the sums
over ranks go in (pp3_eval_column_sums -> Comm.sum_ranks_device -> pp3_eval_finish, once for the means
and once for the squared deviations: two all-gathers of 22 floats, summed in rank order, the same bits
on every rank), still with one host wait.  Every env of the job weighs the same, so ragged shards are
exact; Brax's pmean of per-device means weighs the devices equally instead (the same when the shards
are equal).  `eval/sps` counts all ranks' envs; aggregate_episodes=False stays this rank's columns.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Any, Dict, Optional

import numpy as np

from . import _abi, _lib, rng
from .wrappers import AutoResetEpisodeEnv

METRIC_NAMES = ("total_dist",) + _abi.REWARD_NAMES + ("reward",)  # the accumulator's 20 episode_metrics columns


class Evaluator:
    """See the module docstring.  `eval_env`: a `wrappers.wrap`ped env that this object drives from
    now on (every evaluation resets it); `episode_length` and `action_repeat` must be the wrapper's.
    `key`: a jax-style uint32[2]; every evaluation consumes one split of it.  `comm`: the mean / std
    keys cover all ranks' eval envs (module docstring); None: this process's envs, with the launches
    of a build without it."""

    def __init__(self, eval_env, policy, episode_length: int, action_repeat: int = 1, key=None,
                 deterministic: bool = True, metrics: bool = True, chunk: int = 50, comm=None):
        if not isinstance(eval_env, AutoResetEpisodeEnv):
            raise ValueError("the Evaluator needs a wrapped env (wrappers.wrap: EpisodeWrapper + AutoResetWrapper)")
        if (int(episode_length), int(action_repeat)) != (eval_env.episode_length, eval_env.action_repeat):
            raise ValueError(f"episode_length {episode_length} / action_repeat {action_repeat} are not the eval env's "
                             f"({eval_env.episode_length} / {eval_env.action_repeat})")
        if key is None:
            raise ValueError("the Evaluator needs a key")
        if int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        self.env, self.base = eval_env, eval_env.env
        self.policy = policy
        self.episode_length, self.action_repeat = int(episode_length), int(action_repeat)
        self.unroll = self.episode_length // self.action_repeat
        if self.unroll < 1:
            raise ValueError("episode_length // action_repeat must be >= 1")
        self.deterministic, self.metrics = bool(deterministic), bool(metrics)
        self.chunk = 1 if self.metrics else min(int(chunk), self.unroll)
        self._key = np.array(np.asarray(key, dtype=np.uint32).reshape(2))
        self._L = _lib.load()
        n, dev = self.base.num_envs, self.base.device
        self.num_envs = n
        self._acc = _lib.DeviceBuffer(4 * _abi.EVAL_WORDS * n, dev)
        self.comm = comm
        # out42, then with comm the rank-summed 22 (downloaded with it: the global env count) and this rank's 22
        self._out = _lib.DeviceBuffer(4 * (2 * _abi.EVAL_NOUT + (2 * _abi.EVAL_WORDS if comm is not None else 0)), dev)
        self._actions = _lib.DeviceBuffer(4 * self.chunk * n * _abi.NU, dev)
        self._rows = None if self.metrics else (_lib.DeviceBuffer(4 * self.chunk * n, dev),
                                                _lib.DeviceBuffer(4 * self.chunk * n, dev))
        self._walltime = 0.0

    # ---- launches ---------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        _lib.check(rc, "ppo")

    def _unroll_chunk(self, policy, nsteps: int, key, reward, done):
        """nsteps wrapper steps with the policy in the loop, no observation trajectory; -> the next key."""
        base, L = self.base, self._L
        if self.deterministic:
            _lib.check(L.pp3_rollout_policy(base._h, policy._h, nsteps, self._actions.ptr, reward, done, None, None))
            return key
        k_out = np.zeros(2, dtype=np.uint32)
        _lib.check(L.pp3_rollout_policy_sample(base._h, policy._h, nsteps, key.ctypes.data_as(C.c_void_p),
                                               k_out.ctypes.data_as(C.c_void_p), self._actions.ptr, None, None, reward,
                                               done, None, None))
        return k_out

    def _accumulate(self, policy, key) -> None:
        """The whole unroll behind a device-side reset, accumulated into self._acc (nothing waits)."""
        base, L = self.base, self._L
        n, dev = self.num_envs, base.device
        stream = C.c_void_p(L.pp3_stream(base._h))
        base._keys_buf.upload(np.ascontiguousarray(rng.split(key, n, base._partitionable)))
        base.reset_device(base._keys_buf.ptr.value)
        self.env._first_ps = self.env._first_obs = None  # (the wrapper's host copies of the last reset)
        self._check(L.pp3_eval_reset(dev, n, self._acc.ptr, stream))
        key = np.ascontiguousarray(key)
        if self.metrics:
            fld = {f: base.device_field(f) for f in (_abi.F_REWARD, _abi.F_DONE, _abi.F_METRICS, _abi.F_EPISODE)}
            p = lambda f: C.c_void_p(fld[f][0])  # noqa: E731
            for _ in range(self.unroll):
                key = self._unroll_chunk(policy, 1, key, None, None)
                self._check(L.pp3_eval_accumulate(dev, n, p(_abi.F_REWARD), p(_abi.F_DONE), p(_abi.F_METRICS),
                                                  fld[_abi.F_METRICS][1], p(_abi.F_EPISODE), fld[_abi.F_EPISODE][1],
                                                  self._acc.ptr, stream))
        else:
            reward, done = (b.ptr for b in self._rows)
            t = 0
            while t < self.unroll:
                k = min(self.chunk, self.unroll - t)
                key = self._unroll_chunk(policy, k, key, reward, done)
                self._check(L.pp3_eval_accumulate_rows(dev, k, n, n, reward, done, t, self.action_repeat,
                                                       self._acc.ptr, stream))
                t += k

    def accumulators(self) -> np.ndarray:
        """The last evaluation's accumulator, downloaded: f32 [22][N] (waits for the stream)."""
        self.base.synchronize()
        out = np.empty((_abi.EVAL_WORDS, self.num_envs), np.float32)
        self._acc.download(out)
        return out

    # ---- the Evaluator's surface ------------------------------------------------------------
    def run_evaluation(self, training_metrics: Optional[Dict[str, Any]] = None, aggregate_episodes: bool = True,
                       policy=None) -> Dict[str, Any]:
        """One evaluation with `policy` (default: the constructor's).  Keys: `self._key, k = split(self._key)`;
        the envs reset with split(k, N); a sampled unroll starts its chain from k.  Returns
        eval/episode_<name> and eval/episode_<name>_std for METRIC_NAMES (metrics=False: reward only),
        eval/avg_episode_length, eval/std_episode_length, eval/epoch_eval_time, eval/sps, eval/walltime and
        `training_metrics` merged in.  aggregate_episodes=False: eval/episode_<name> are the per-env
        columns [N] instead (no _std keys), with eval/episode_steps and eval/active_episodes [N]."""
        policy = self.policy if policy is None else policy
        base, L = self.base, self._L
        t0 = time.time()
        part = base._partitionable
        self._key, k = (np.array(x) for x in rng.split(self._key, 2, part))
        self._accumulate(policy, k)
        stream = L.pp3_stream(base._h)
        total_envs = self.num_envs
        if self.comm is None:
            self._check(L.pp3_eval_reduce(base.device, self.num_envs, self._acc.ptr, self._out.ptr, C.c_void_p(stream)))
            base.synchronize()  # the evaluation's one host wait
            out = np.empty(2 * _abi.EVAL_NOUT, np.float32)
            self._out.download(out)
        else:
            out42 = self._out.ptr.value
            total, local = out42 + 4 * 2 * _abi.EVAL_NOUT, out42 + 4 * (2 * _abi.EVAL_NOUT + _abi.EVAL_WORDS)
            for which, mean in ((0, None), (1, C.c_void_p(out42))):
                self._check(L.pp3_eval_column_sums(base.device, self.num_envs, self._acc.ptr, mean, C.c_void_p(local),
                                                   C.c_void_p(stream)))
                self.comm.sum_ranks_device(local, total, _abi.EVAL_WORDS, stream)
                self._check(L.pp3_eval_finish(base.device, C.c_void_p(total), which, C.c_void_p(out42),
                                              C.c_void_p(stream)))
            base.synchronize()  # the evaluation's one host wait
            out = np.empty(2 * _abi.EVAL_NOUT + _abi.EVAL_WORDS, np.float32)
            self._out.download(out)
            total_envs = int(out[-1])  # (the rank sum of the shard sizes, exact in f32)
        mean, std = out[:_abi.EVAL_NOUT], out[_abi.EVAL_NOUT:2 * _abi.EVAL_NOUT]
        cols = range(_abi.EVAL_NCOL) if self.metrics else (_abi.EVAL_NCOL - 1,)
        res: Dict[str, Any] = {}
        if aggregate_episodes:
            for c in cols:
                res[f"eval/episode_{METRIC_NAMES[c]}"] = float(mean[c])
                res[f"eval/episode_{METRIC_NAMES[c]}_std"] = float(std[c])
        else:
            acc = self.accumulators()
            for c in cols:
                res[f"eval/episode_{METRIC_NAMES[c]}"] = acc[c].copy()
            res["eval/episode_steps"] = acc[_abi.EVAL_STEPS].copy()
            res["eval/active_episodes"] = acc[_abi.EVAL_ACTIVE].copy()
        res["eval/avg_episode_length"] = float(mean[_abi.EVAL_NOUT - 1])
        res["eval/std_episode_length"] = float(std[_abi.EVAL_NOUT - 1])
        dt = time.time() - t0
        self._walltime += dt
        res["eval/epoch_eval_time"] = dt
        res["eval/sps"] = total_envs * self.unroll * self.action_repeat / dt
        res["eval/walltime"] = self._walltime
        res.update(training_metrics or {})
        return res

    def state_dict(self) -> Dict[str, np.ndarray]:
        """{"key": the key the next evaluation splits}: all an Evaluator carries from one evaluation to
        the next (every evaluation resets its envs and its accumulator; the walltime is a timing)."""
        return {"key": self._key.copy()}

    def load_state_dict(self, d: Dict[str, np.ndarray]) -> None:
        key = np.asarray(d["key"])
        if key.dtype != np.uint32 or key.shape != (2,):
            raise ValueError("the Evaluator's state_dict holds key: uint32 [2]")
        self._key = np.array(key)

    def close(self) -> None:
        for b in (self._acc, self._out, self._actions) + (self._rows or ()):
            b.free()
