"""Cost of one PPO evaluation (evaluator.Evaluator.run_evaluation: reset, unroll of `--steps` wrapper
steps with the policy in the loop, accumulate, reduce, one download) after `--warmup` warm-up steps,
in wall-clock ms from call to return (every timed piece ends with the wait for the device), medians
over `--repeat` alternating rounds with the run-to-run spread (min .. max) beside them.  Per env count
of `--envs` and per actor (deterministic: tanh of the mean, pp3_rollout_policy; sampled:
pp3_rollout_policy_sample), in the same rounds:
  eval_metrics_ms   the metrics path: one-step launches, pp3_eval_accumulate behind each (20 columns);
  eval_reward_ms    the reward path: launches of `--chunk` steps, pp3_eval_accumulate_rows behind each;
  bare_steps_ms     (a) the metrics path's reset and launches without any accumulation or reduce;
  bare_chunks_ms    (a) the same for the reward path;
  parent_numpy_ms   (b) what the library offers without the evaluator for the reward path's numbers:
                    wrap(env).rollout_policy[_sample] in unrolls of `--chunk` steps, the trajectories
                    downloaded, EvalWrapper's recurrence on reward and done in numpy, np.mean / np.std.
"share" is the accumulation's part of an evaluation, 1 - bare / eval.  "agree": the reward path's
reward and length numbers equal the metrics path's bit for bit, and the numpy accumulation's mean
reward lies within the summation bound of tests/test_ppo_eval_ref.py of the device's.
One child process under a time limit; the result line is printed and appended to `--out`.

  python tools/ppo_eval_bench.py [--envs 4096,128 --steps 1000 --warmup 200 --chunk 50 --repeat 9 --timeout 900]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pupperv3-mjx_amd"), os.path.join(ROOT, "tests")]


def child(envs, T: int, W: int, chunk: int, R: int) -> None:
    from collections import OrderedDict
    from types import SimpleNamespace

    import numpy as np

    import bench
    from pupperv3_mjx import MODEL_XML, _abi, evaluator, export, rng, wrappers
    from pupperv3_mjx.environment import PupperV3Env

    rs = np.random.RandomState(7)
    result = {"steps": T, "warmup": W, "chunk": chunk, "rounds": R, "configs": []}
    for E in envs:
        env = PupperV3Env(**bench.bench_kwargs(MODEL_XML), num_envs=E, device=0, pipeline_output=False)
        w = wrappers.wrap(env, episode_length=T)
        D = env.observation_size
        sizes = [D, 256, 128, 128, 2 * _abi.NU]
        layers = OrderedDict((f"hidden_{i}", {"kernel": rs.normal(scale=1 / np.sqrt(sizes[i]), size=(sizes[i], sizes[i + 1])),
                                              "bias": np.zeros(sizes[i + 1])}) for i in range(len(sizes) - 1))
        params = (SimpleNamespace(mean=np.zeros(D), std=np.ones(D)), {"params": layers})
        args = ("elu", 0.75, 5.0, 0.25, np.zeros(12), np.ones(12), -np.ones(12), True, env._observation_history, 30.0, 30.0)
        pols = {False: export.DevicePolicy(export.convert_params(params, *args)),
                True: export.DevicePolicy(export.convert_training_params(params, *args))}
        key = np.array(rng.PRNGKey(1), dtype=np.uint32)
        st = w.reset(np.ascontiguousarray(rng.split(rng.PRNGKey(0), E)))
        for w0 in range(0, W, 20):  # (in unrolls of 20: the trajectory each one returns stays small)
            st, _, key = w.rollout_policy_sample(st, pols[True], min(20, W - w0), key)
        del st
        for sampled in (False, True):
            pol = pols[sampled]
            k_eval = np.array(rng.PRNGKey(3), dtype=np.uint32)
            ev = {name: evaluator.Evaluator(w, pol, T, key=k_eval, deterministic=not sampled, metrics=m, chunk=chunk)
                  for name, m in (("metrics", True), ("reward", False))}

            def run(name):
                ev[name]._key = k_eval.copy()  # every round evaluates the same episodes
                return ev[name].run_evaluation()

            def bare(name):
                e = ev[name]
                k = np.ascontiguousarray(rng.split(k_eval, 2, env._partitionable)[1])
                env._keys_buf.upload(np.ascontiguousarray(rng.split(k, E, env._partitionable)))
                env.reset_device(env._keys_buf.ptr.value)
                rows = (None, None) if e.metrics else tuple(b.ptr for b in e._rows)
                t = 0
                while t < T:
                    n = min(e.chunk, T - t)
                    k = e._unroll_chunk(pol, n, k, *rows)
                    t += n
                env.synchronize()

            def parent():
                """-> (mean, std) of episode reward and length, EvalWrapper's recurrence in numpy f32"""
                k = rng.split(k_eval, 2, env._partitionable)[1]
                s = w.reset(np.ascontiguousarray(rng.split(k, E, env._partitionable)))
                em, active, es = np.zeros(E, np.float32), np.ones(E, np.float32), np.zeros(E, np.float32)
                t = 0
                while t < T:
                    n = min(chunk, T - t)
                    if sampled:
                        s, traj, k = w.rollout_policy_sample(s, pol, n, k)
                    else:
                        s, traj = w.rollout_policy(s, pol, n)
                    for j in range(n):
                        es = np.where(active != 0, np.float32(t + j + 1), es)
                        em = em + traj["reward"][j] * active
                        active = active * (np.float32(1) - traj["done"][j])
                    t += n
                return float(np.mean(em)), float(np.std(em)), float(np.mean(es)), float(np.std(es)), em

            pieces = OrderedDict((("eval_metrics_ms", lambda: run("metrics")), ("eval_reward_ms", lambda: run("reward")),
                                  ("bare_steps_ms", lambda: bare("metrics")), ("bare_chunks_ms", lambda: bare("reward")),
                                  ("parent_numpy_ms", parent)))
            last = {name: fn() for name, fn in pieces.items()}  # one untimed pass of everything
            times = {name: [] for name in pieces}
            names = list(pieces)
            for r in range(R):
                for name in names[r % len(names):] + names[:r % len(names)]:  # the order rotates
                    t0 = time.perf_counter()
                    last[name] = pieces[name]()
                    times[name].append(1e3 * (time.perf_counter() - t0))
            med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
            m, rwd, par = last["eval_metrics_ms"], last["eval_reward_ms"], last["parent_numpy_ms"]
            same = ("eval/episode_reward", "eval/episode_reward_std", "eval/avg_episode_length", "eval/std_episode_length")
            bound = (math.ceil(E / 1024) + 12) * 2.0 ** -24 * float(np.abs(par[4]).mean())
            # (numpy's pairwise mean carries its own error of the same order: twice the bound)
            result["configs"].append({
                "envs": E, "sampled": sampled, "median_ms": med,
                "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
                "share": {"metrics_path": round(1 - med["bare_steps_ms"] / med["eval_metrics_ms"], 4),
                          "reward_path": round(1 - med["bare_chunks_ms"] / med["eval_reward_ms"], 4)},
                "eval_over_parent": {"metrics_path": round(med["eval_metrics_ms"] / med["parent_numpy_ms"], 4),
                                     "reward_path": round(med["eval_reward_ms"] / med["parent_numpy_ms"], 4)},
                "env_steps_per_s": {"metrics_path": round(E * T / (med["eval_metrics_ms"] * 1e-3)),
                                    "reward_path": round(E * T / (med["eval_reward_ms"] * 1e-3))},
                "episode_reward": m["eval/episode_reward"], "episode_reward_std": m["eval/episode_reward_std"],
                "avg_episode_length": m["eval/avg_episode_length"],
                "agree": {"reward_path_equals_metrics_path": all(m[k] == rwd[k] for k in same),
                          "numpy_mean_reward_within_bound": abs(par[0] - m["eval/episode_reward"]) <= 2 * bound,
                          "numpy_mean_length_equal": par[2] == m["eval/avg_episode_length"]}})
            for e in ev.values():
                e.close()
        for p in pols.values():
            p.close()
        env.close()
    print(json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,128", help="env counts, comma separated")
    ap.add_argument("--steps", type=int, default=1000, help="episode length = unroll length (action_repeat 1)")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=50, help="steps per launch of the reward path and of (b)")
    ap.add_argument("--repeat", type=int, default=9, help="timed rounds (medians and min .. max are reported)")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_eval_bench.txt"), help="result lines are appended here")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    envs = [int(x) for x in args.envs.split(",")]
    if args.child:
        child(envs, args.steps, args.warmup, args.chunk, args.repeat)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", args.envs, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--chunk", str(args.chunk), "--repeat", str(args.repeat)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {args.timeout} s", file=sys.stderr)
        return 124
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-2000:])
        return out.returncode
    line = out.stdout.strip().split("\n")[-1]
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
